"""One record set per positions-per-lane class for the per-column and sliced EM kernels (helper; not collected by pytest).

k_em_seq, k_e_slice, k_m_slice and k_m_list (csrc/kernels.hip) are instantiated once per class of csrc/mclass.h, and their
code differs by class: the E chain read column by column above 16 positions per lane, 16-byte r stores and loads for whole
lanes at a multiple of four, N exceptions patched by an indexed register write at 10..32, the sparse M-step up to 16, the
list walk's prefetch of four batches.  class_set(orc, flavour, M) builds the records that put a class's lane edges under
all of them; tests/test_em_classes_cpu.py pins what is claimed here without a GPU, tests/test_em_classes_gpu.py runs them.

Per class (prev = the class before it, 0 for the first; single strand, so a record is as long as written):
  edge     the shortest record max(W, 64 prev + 1), the longest 64 M, 64 M - 1 and one middle length that is a multiple of
           neither 4 nor M, each with N as tests/test_score_classes_gpu.py::with_n places them: at 0, M - 1, M, L - 1 and a
           run of K + 2 across the lane boundary at 32 M (placements beyond the record's end are dropped)
  clean    one record without N: no exception
  single   one record with one interior N: 1..K exceptions, all of them within the kRawExc = 6 that travel with the record
  filler   records of seeded random length inside the class with N at n_frac = 0.002, until the class holds min_records(M):
           under set_launch(blocks=1) every wave then walks at least three records
An N is a random base per k-mer that covers it (Sequence.cpp:34-41), so how many positions become exceptions depends on
libc's rand(): the builder takes the first seed of the encoder, from 42 on, at which the clean record has none, the single
N between 1 and 6 and some edge record that holds the run more than 6 -- counted by the test from PackedSeqs.arrays().

Two models per flavour, both on the same records (a site of the sharp matrix is planted in every record, clear of its N
where a window without N exists):
  blurred  tests/cases.py::Case's v0, a make_pwm matrix blended with the uniform one (0.3, raised where BLEND says so)
  sharp    regimes.sharp_pwm at SHARP's (squarings, q), chosen as regimes.R2_SHAPES chooses them
"""
from __future__ import annotations

import os
import re
from types import SimpleNamespace

import numpy as np

from bammmotif2_amd import synth
from tests import regimes
from tests.test_score_classes_gpu import M_CLASSES, with_n
from tests.test_score_tiles_gpu import bases

# P: k_em_seq under grouped=0; S: the sliced path; L: the sliced path at a width that leaves the list walk room in the long
# classes.  At W = 30 the count table is cut into two slices of 15 columns (123 000 bytes), and from 40 positions per lane on a
# block's copies of the decoded records (8 waves of 64 M + 8 shorts: 41 088 bytes at M = 40) no longer fit beside one: the
# planner then walks dense r whatever the tuning says (csrc/em_pass.cpp: sliced_geometry), and k_m_list's seven longest
# instantiations run nowhere in flavour S.  At W = 20 the slices hold 10 columns and every class fits.
FLAVOURS = {"P": dict(K=2, W=20), "S": dict(K=4, W=30), "L": dict(K=4, W=20)}
LIST_FITS_UP_TO = 32                                         # flavour S: the longest class whose `list` tuning reaches k_m_list
MODELS = ("blurred", "sharp")
ALPHA_BG = np.array([1.0, 10.0, 10.0], np.float32)
BG_ORDER = 2
N_FRAC = 0.002
PWM_SEED = 7                                                 # Case's default seed: make_pwm and sharp_pwm draw the same weights
Q = 0.3
NONZERO = 2.0 ** -40                                         # "non-zero" in fp64: r * 2^40 >= 1, the M-step's addend is not 0
RAW_EXC = 6                                                  # device_utils.h: kRawExc
LIST_PREFETCH = 256                                          # kernels.hip: k_m_list's NP = 4 batches of 64 entries

# blend of the blurred model with the uniform matrix: Case's 0.3 unless a (flavour, M) needs more for the gate's condition
# (every record with more than 256 windows has more than 256 non-zero windows)
BLEND_DEFAULT = 0.3
#   W = 30 at 5 and 6 positions per lane: records of 257..384 positions have 228..355 windows, and at 0.3 up to 91 of them
#   fall below 2^-40; at 0.5 every window adds
BLEND: dict = {("S", 5): 0.5, ("S", 6): 0.5}
# (squarings, q) of the sharp model, as regimes.R2_DEFAULT; per (flavour, M) where the gate's conditions need another
SHARP_DEFAULT = (5, 0.3)
SHARP: dict = {}


def classes_of(flavour: str):
    """The classes a flavour is built for: all 23, or -- flavour L -- the ones flavour S cannot take through k_m_list."""
    return [M for M in M_CLASSES if M > LIST_FITS_UP_TO] if flavour == "L" else list(M_CLASSES)


def prev_class(M: int) -> int:
    i = M_CLASSES.index(M)
    return M_CLASSES[i - 1] if i else 0


def threads_for(M: int) -> int:
    """The class's block size (csrc/mclass.h; the gate compares this with the header's table)."""
    return 1024 if M <= 8 else 768 if M <= 20 else 512 if M <= 64 else 256


def mclass_table():
    """[(M, threads)] as csrc/mclass.h lists them."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bammmotif2_amd", "csrc", "mclass.h")
    return [(int(m), int(t)) for m, t in re.findall(r"X\(\d+,\s*(\d+),\s*(\d+)\)", open(path).read())]


def min_records(M: int) -> int:
    """3 T / 64 + 1 records: one block's waves walk three each and one wave a fourth.  The list walk of the 16-per-lane class
    runs 16 waves per block whatever the class's own block size is (kernels.hip: launch_m_list), so that class counts 1024."""
    T = max(threads_for(M), 1024) if M == 16 else threads_for(M)
    return 3 * T // 64 + 1


def edge_lengths(M: int, W: int):
    prev = prev_class(M)
    lo, hi = max(W, 64 * prev + 1), 64 * M
    mid = (lo + hi) // 2
    while mid % 4 == 0 or (M > 1 and mid % M == 0):          # (every length is a multiple of 1)
        mid += 1
    assert lo < mid < hi - 1
    return [lo, hi, hi - 1, mid]


def _plant(rec, site, rs):
    """The site at a window of the record that holds no N; where there is none, at any window, the N put back on top."""
    W, L = len(site), len(rec)
    n_at = rec == 0
    for _ in range(64):
        s = int(rs.randint(0, L - W + 1))
        if not n_at[s:s + W].any():
            break
    rec[s:s + W] = site
    rec[n_at] = 0
    return rec


def class_records(flavour: str, M: int):
    """([codes], [kind]) of one class: the four edge records, the clean one, the single-N one, the fillers."""
    K, W = FLAVOURS[flavour]["K"], FLAVOURS[flavour]["W"]
    seed = 100 * M_CLASSES.index(M) + {"P": 0, "S": 50, "L": 25}[flavour]
    rs = np.random.RandomState(7000 + seed)
    lo, hi = max(W, 64 * prev_class(M) + 1), 64 * M
    recs, kinds = [], []
    for i, L in enumerate(edge_lengths(M, W)):
        recs.append(with_n(L, M, K, 1000 + seed + i)); kinds.append("edge")
    recs.append(bases(int(rs.randint(lo, hi + 1)), 2000 + seed)); kinds.append("clean")
    one = bases(int(rs.randint(max(lo, W + 2), hi + 1)), 3000 + seed)
    one[len(one) // 2] = 0
    recs.append(one); kinds.append("single")
    while len(recs) < min_records(M):
        r = bases(int(rs.randint(lo, hi + 1)), 4000 + seed + len(recs))
        r[rs.random_sample(len(r)) < N_FRAC] = 0
        recs.append(r); kinds.append("filler")
    # a site of the sharp matrix in every record (the draws of synth.make_sequences, one record at a time)
    squarings, _ = SHARP.get((flavour, M), SHARP_DEFAULT)
    cdf = np.cumsum(regimes.sharp_pwm(W, PWM_SEED, squarings).astype(np.float64), axis=0)
    for r in recs:
        site = (rs.random_sample(W)[None, :] > cdf[:3, :]).sum(axis=0).astype(np.uint8) + 1
        _plant(r, site, rs)
    return recs, kinds


def exception_counts(arrays: dict, K: int) -> np.ndarray:
    """Per record, the exceptions the order-K kernels patch: the entries of PackedSeqs.arrays() whose k-mer differs from what
    the 2-bit stream implies within the lowest K + 1 digits (csrc/seqs.cpp builds the device's list the same way)."""
    differs = ((arrays["exc_kmer"] ^ arrays["exc_clean"]) & np.uint32(4 ** (K + 1) - 1)) != 0
    at = np.concatenate([[0], np.cumsum(differs)])
    return (at[arrays["exc_off"][1:].astype(np.int64)] - at[arrays["exc_off"][:-1].astype(np.int64)]).astype(np.int64)


def kmer_exception_counts(kmer, off, K: int) -> np.ndarray:
    """The same count from the encoder's k-mers alone: positions whose digits 1..K are not the bases (digit 0) of the
    positions before them."""
    out = np.zeros(len(off) - 1, np.int64)
    for n in range(len(off) - 1):
        km = kmer[int(off[n]):int(off[n + 1])].astype(np.int64)
        base = km & 3
        bad = np.zeros(len(km), bool)
        for d in range(1, K + 1):
            bad[d:] |= ((km[d:] >> (2 * d)) & 3) != base[:-d]
        out[n] = int(bad.sum())
    return out


class ClassSet:
    """The records of one (flavour, class), encoded by the oracle, with the background learned from them."""

    def __init__(self, orc, flavour: str, M: int):
        self.flavour, self.M, self.prev = flavour, M, prev_class(M)
        self.K, self.W, self.bg_order = FLAVOURS[flavour]["K"], FLAVOURS[flavour]["W"], BG_ORDER
        self.name = f"{flavour}{M}"
        self.records, self.kinds = class_records(flavour, M)
        self.N = len(self.records)
        in_off = np.concatenate([[0], np.cumsum([len(r) for r in self.records])]).astype(np.uint64)
        codes = np.concatenate(self.records)
        kinds = np.array(self.kinds)
        with_run = np.array([k == "edge" and len(r) >= 32 * M + self.K + 2 for k, r in zip(self.kinds, self.records)])
        for self.encoder_seed in range(42, 74):
            _, self.kmer, self.off = orc.encode_set(codes, in_off, True, self.encoder_seed)
            exc = kmer_exception_counts(self.kmer, self.off, self.K)
            if exc[kinds == "clean"][0] == 0 and 1 <= exc[kinds == "single"][0] <= RAW_EXC and exc[with_run].max() > RAW_EXC:
                break
        else:
            raise AssertionError(f"{self.name}: no encoder seed gives the three exception counts")
        self.many = int(np.flatnonzero(with_run)[np.argmax(exc[with_run])])       # the edge record with the most exceptions
        self.clean, self.single = int(np.flatnonzero(kinds == "clean")[0]), int(np.flatnonzero(kinds == "single")[0])
        self.vbg = orc.bg_model(self.kmer, self.off, self.bg_order, ALPHA_BG)
        self.A = synth.alpha_matrix(synth.default_alpha(self.K), self.W)
        for a in (self.kmer, self.off, self.vbg, self.A):
            a.setflags(write=False)

    def model(self, which: str):
        """(v, q) of `blurred` or `sharp`."""
        if which == "blurred":
            b = BLEND.get((self.flavour, self.M), BLEND_DEFAULT)
            pwm = synth.make_pwm(self.W, PWM_SEED)
            return synth.bamm_from_pwm(((1.0 - b) * pwm + b * 0.25).astype(np.float32), self.K), Q
        squarings, q = SHARP.get((self.flavour, self.M), SHARP_DEFAULT)
        return synth.bamm_from_pwm(regimes.sharp_pwm(self.W, PWM_SEED, squarings), self.K), q

    def inputs(self, which: str, keep=None) -> regimes.Inputs:
        """regimes.Inputs of the model on the whole set, or on the records `keep` alone (same background: a fold's mask
        does not re-learn it)."""
        v, q = self.model(which)
        kmer, off = self.kmer, self.off
        if keep is not None:
            kmer, off = subset(self.kmer, self.off, keep)
        case = SimpleNamespace(K=self.K, W=self.W, bg_order=self.bg_order, name=self.name)
        return regimes.Inputs(case, kmer, off, v, q, self.A, self.vbg)


def subset(kmer, off, keep):
    o = off.astype(np.int64)
    sub = np.concatenate([kmer[o[n]:o[n + 1]] for n in keep])
    return sub, np.concatenate([[0], np.cumsum(np.diff(o)[keep])]).astype(np.uint64)


def fold_mask(N: int) -> np.ndarray:
    """Every third record dropped, the first and the last included."""
    mask = (np.arange(N) % 3 != 0).astype(np.uint8)
    mask[-1] = 0
    return mask


def nonzero_windows(inp: regimes.Inputs, r64) -> np.ndarray:
    """Per record, the windows whose fp64 r makes a non-zero addend."""
    off = inp.off.astype(np.int64)
    return np.array([int((r64[off[n]:off[n + 1]] >= NONZERO).sum()) for n in range(inp.N)])


_SETS: dict = {}
_CASES: dict = {}


def class_set(orc, flavour: str, M: int) -> ClassSet:
    if (flavour, M) not in _SETS:
        _SETS[(flavour, M)] = ClassSet(orc, flavour, M)
    return _SETS[(flavour, M)]


def case(orc, flavour: str, model: str, M: int):
    """(Inputs, regimes.Reference) of one (flavour, model, class): computed once, shared, never modified."""
    key = (flavour, model, M)
    if key not in _CASES:
        inp = class_set(orc, flavour, M).inputs(model)
        _CASES[key] = (inp, regimes.Reference(orc, inp))
    return _CASES[key]


# ---------------------------------------------------------------------------- bars --

def pair_name(flavour: str, model: str) -> str:
    """The `regime` under which regimes.PAIR_BARS lists a (flavour, model); the shape is the class set's name, e.g. S128."""
    return f"em_classes_{flavour}_{model}"


def bars(flavour: str, model: str, inp: regimes.Inputs) -> dict:
    """{quantity: (rtol, atol)} of the comparison with fp64: tests/regimes.py's bars as they stand, and twice the gate's
    figure where regimes.PAIR_BARS lists the pair (the ratio atol / rtol kept, as regimes.v_bar keeps it)."""
    base = {"r": (regimes.R_RTOL * regimes.r_len_factor(inp.off), regimes.R_ATOL), "llh": (regimes.LLH_RTOL, regimes.llh_atol(inp.N)),
            "counts": (regimes.N_RTOL, regimes.N_ATOL), "v": (regimes.V_RTOL, regimes.V_ATOL)}
    out = {}
    for k, (rtol, atol) in base.items():
        wide = max(rtol, regimes.PAIR_BARS.get((pair_name(flavour, model), inp.case.name, k), 0.0))
        out[k] = (wide, atol * (wide / rtol))
    assert out["v"] == regimes.v_bar(pair_name(flavour, model), inp.case.name)
    return out
