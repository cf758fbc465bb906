"""One record set per case for the fused model update (helper; not collected by pytest).

Inside iterate() / optimize() a handle with K <= 2 runs the update of pass p in the block prologue of pass p + 1's first
grouped or mixed-row launch (csrc/update_kernel.h, called from grouped_kernel.h and mixed_kernel.h).  The prologue is compiled
into k_em_grp's eleven classes of 2..16 positions per lane and into k_em_mix / k_em_mix1 at 4..10; SPECS names one case per
(family, class) of them, tests/test_fused_classes_cpu.py pins what is claimed here without a GPU and
tests/test_fused_classes_gpu.py runs them.

A set for class M (prev = the class before it) holds 4 T / 64 + 1 records, T the class's block size: under
Context.set_launch(blocks=2) the launch then has a writer block and another one, every wave walks two records and one a third.
  edge     both strands: 32 prev and 32 M - 1 bases (64 prev + 1 and 64 M - 1 positions); single strand: 64 prev + 1, 64 M and
           64 M - 1
  clean    one record of a middle length
  single   single strand only: one record with one interior N in its middle, K + G + 2 positions or more from both ends.  A
           record on both strands carries its junction's exceptions already, and an N anywhere else makes a second and a third
           stretch of them (the N and its mirror image), which xrec_for_group's one range lo..lo + B - 1 does not hold: such a
           record leaves the grouped launch for k_em_seq and plan() is no longer (N, 0, 1).  The sets on both strands hold one
           filler more instead.
  filler   clean records of seeded lengths inside the class
Every record carries a planted site of the case's matrix.  The background is the oracle's at order 2, the model Case's blend
0.7 pwm + 0.3 uniform at q = 0.3.

Mixed rows: a record RUNS in the shortest class whose 64 M slots reach its span L - W + 3 + 3 (4 - B) (csrc/plan.cpp:
plan_class_split; tests/test_mix_anchor_gpu.py), start-anchored, if that class is shorter than the class of its length; else
in the class of its length, end-anchored.  One launch means one class of the length and one class of the span, so a
start-anchored set for class M holds lengths of 64 M + 1 .. 64 M + c only (c = L - span = W - 3 - 3 (4 - B): 5..17
positions, three to nine odd lengths), its shortest and longest at both ends of that range: spans of 64 M + 1 - c .. 64 M.  An
end-anchored set (`mix_anchor` = 0) takes every odd length of the class.  The class of 10 positions per lane is never the
target of the anchor rule -- the class above it, 12, has no mixed rows (mix_geometry), so no bucket exists whose records could
move down to 10; tests/test_mix_anchor_gpu.py::test_a_class_12_bucket_is_no_mixed_row_launch pins that -- and appears
end-anchored only.
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from bammmotif2_amd import synth
from tests import regimes
from tests.em_classes import M_CLASSES, _plant, kmer_exception_counts, prev_class, subset
from tests.test_score_tiles_gpu import bases

FUSED_CLASSES = [M for M in M_CLASSES if 2 <= M <= 16]       # grouped_kernel.h: BAMM_FUSE_MAX_M
MIXED_CLASSES = [4, 5, 6, 7, 8, 10]                          # grouped.hip: mix_geometry
P = 4                                                        # passes per case: within the five of the q window either way
ALPHA_BG = np.array([1.0, 10.0, 10.0], np.float32)
BG_ORDER = 2
PWM_SEED = 7
Q = 0.3
BLEND = 0.3
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bammmotif2_amd", "csrc")


def threads_for(M: int) -> int:
    """Block size of the grouped and mixed-row kernels of a fused class."""
    return 1024 if M <= 8 else 768


def grp_max_threads_source():
    """grp_max_threads as csrc/grouped.hip writes it: a function of M read from the chain of `M <= a ? b : ...`."""
    text = open(os.path.join(CSRC, "grouped.hip")).read()
    (expr,) = re.findall(r"uint32_t grp_max_threads\(int M\) \{ return (.*?); \}", text)
    steps = [(int(a), int(b)) for a, b in re.findall(r"M <= (\d+) \? (\d+)u", expr)]
    (last,) = re.findall(r": (\d+)u\)*$", expr)
    assert steps and steps == sorted(steps)
    return lambda M: next((t for a, t in steps if M <= a), int(last))


def n_records(M: int) -> int:
    return 4 * threads_for(M) // 64 + 1


def class_of(L: int) -> int:
    return next(M for M in M_CLASSES if 64 * M >= L)


def mix_groups(W: int):
    """(A wide groups, B narrow groups): W = 3 B + 4 A with A = W mod 3."""
    A = W % 3
    return A, (W - 4 * A) // 3


def mix_span(L: int, W: int) -> int:
    return L - W + 3 + 3 * (4 - mix_groups(W)[1])


def run_class(L: int, W: int, anchor: bool) -> int:
    """The class a record of L positions runs in under mixed rows: the span's class when that is shorter than the length's
    and has mixed rows, else the length's."""
    own = class_of(L)
    if not anchor:
        return own
    need = -(-mix_span(L, W) // 64)
    cand = next((M for M in MIXED_CLASSES if M >= need), None)
    return cand if cand is not None and cand < own else own


@dataclass(frozen=True)
class Spec:
    name: str
    K: int
    W: int
    M: int                                                   # the class the first launch runs in
    ss: bool = False
    tune: tuple = ()                                         # (key, value) of Context.set_tuning while the handles are created
    mixed: bool = False
    anchored: bool = False
    fusable: bool = True                                     # what plan_update() must report under fused_update = 1
    form: int = 0
    plan: tuple = None                                       # plan() where it is not (N, 0, 1)
    stop: bool = False                                       # also runs optimize() to its stop rule
    why: str = ""

    @property
    def tuning(self) -> dict:
        return dict(self.tune)


def _uniform(name, K, W, M, ss=False, **kw):
    return Spec(name=name, K=K, W=W, M=M, ss=ss, **kw)


def _mixed(W, M, anchored):
    A = mix_groups(W)[0]
    return Spec(name=f"mix_a{A}_w{W}_m{M}_{'start' if anchored else 'end'}", K=2, W=W, M=M, mixed=True, anchored=anchored,
                tune=(("group_layout", 8), ("mix_anchor", int(anchored))), stop=(W, M, anchored) == (20, 6, True))


# Class 2 at K = 2 takes G = 2 only (a group is no wider than a lane's run), and W = 20 still plans there (T = 10 groups:
# (Bj + edge) T = 60 fix lanes of the 64); the CPU test holds the set's shortest record, 65 positions, against W.
SPECS = (
    # uniform rows, both strands, K = 2, W = 20: all eleven classes
    [_uniform(f"u_k2_w20_m{M}", 2, 20, M, stop=M in (7, 12)) for M in FUSED_CLASSES]
    # G = 2 at K = 2: forced at W = 20, the planner's own choice at W = 31 (G = 3 does not fit the LDS there)
    + [_uniform(f"g2_k2_w20_m{M}", 2, 20, M, tune=(("group_size", 2),)) for M in (4, 8, 12)]
    + [_uniform(f"g2_k2_w31_m{M}", 2, 31, M) for M in (4, 8, 12)]
    # K = 1, W = 14: G = 4 (3 in the class of 3 positions per lane), and G = 3 forced
    + [_uniform(f"k1_w14_m{M}", 1, 14, M) for M in (3, 7, 10, 16)]
    + [_uniform(f"k1_w14_m{M}_ss", 1, 14, M, ss=True) for M in (5, 14)]
    + [_uniform("k1_w14_m7_g3", 1, 14, 7, tune=(("group_size", 3),)), _uniform("k1_w14_m10_g3_ss", 1, 14, 10, ss=True, tune=(("group_size", 3),))]
    # K = 0, W = 13
    + [_uniform("k0_w13_m6_ss", 0, 13, 6, ss=True), _uniform("k0_w13_m8", 0, 13, 8), _uniform("k0_w13_m12_ss", 0, 13, 12, ss=True)]
    # the table layouts (bits 0-1 of grp_geometry's layout)
    + [_uniform(f"layout{l}_k2_w20_m{M}", 2, 20, M, tune=(("group_layout", l),)) for l in (0, 2, 3) for M in (7, 10)]
    + [_uniform(f"layout{l}_k1_w12_m{M}_ss", 1, 12, M, ss=True, tune=(("group_layout", l),)) for l in (0, 2, 3) for M in (7, 10)]
    # mixed rows, one wide group (W = 13, 16) and two (W = 14, 17, 20), in every class and both flavours
    + [_mixed(W, M, True) for W, M in ((13, 4), (16, 5), (13, 6), (16, 7), (16, 8))]
    + [_mixed(W, M, False) for W, M in ((16, 4), (13, 5), (16, 6), (13, 7), (13, 8), (16, 10))]
    + [_mixed(W, M, True) for W, M in ((14, 4), (17, 5), (20, 6), (14, 7), (17, 8))]
    + [_mixed(W, M, False) for W, M in ((17, 4), (14, 5), (14, 6), (20, 7), (20, 8), (17, 10), (20, 10))]
    # the widths at which plan_fused_update's first line decides: update_fits_lds is 4^(K+1) W <= 2048
    + [_uniform("width_w32_m7", 2, 32, 7, why="plan.cpp plan_fused_update, first line: update_fits_lds(2, 32) holds, 64 * 32 = 2048 exactly"),
       _uniform("width_w33_m7", 2, 33, 7, fusable=False, form=2, plan=(33, 32, 2),
                why="plan.cpp plan_fused_update, first line: update_fits_lds(2, 33) fails (2112 cells), the update runs over blocks; "
                    "T = 17 groups leave two virtual rows per wave, so the records whose junction needs three (32 of the 65) run in k_em_seq"),
       _uniform("width_w1_m7", 2, 1, 7, why="fusable: the one-group count table (off_ng .. off_n1) still holds the update's 844 bytes"),
       _uniform("width_w3_m7", 2, 3, 7, why="fusable: one group of three columns")]
)
SPEC_BY_NAME = {s.name: s for s in SPECS}
assert len(SPEC_BY_NAME) == len(SPECS)


def allowed_lengths(spec: Spec):
    """Every record length (positions) of the case's set, ascending."""
    M, prev = spec.M, prev_class(spec.M)
    if spec.mixed and spec.anchored:
        c = spec.W - 3 - 3 * (4 - mix_groups(spec.W)[1])     # L - span
        lo, hi = 64 * M + 1, 64 * M + c
    else:
        lo, hi = max(spec.W, 64 * prev + 1), 64 * M
    return [L for L in range(lo, hi + 1) if spec.ss or L % 2 == 1]


def edge_lengths(spec: Spec):
    ls = allowed_lengths(spec)
    return [ls[0], ls[-1], ls[-2]] if spec.ss else [ls[0], ls[-1]]


def _records(spec: Spec, rs, seed):
    ls = allowed_lengths(spec)
    n_bases = (lambda L: L) if spec.ss else (lambda L: (L - 1) // 2)
    recs, kinds = [], []
    for i, L in enumerate(edge_lengths(spec)):
        recs.append(bases(n_bases(L), 1000 + seed + i)); kinds.append("edge")
    recs.append(bases(n_bases(ls[len(ls) // 2]), 2000 + seed)); kinds.append("clean")
    if spec.ss:
        one = bases(n_bases(ls[int(rs.randint(len(ls) // 4, len(ls)))]), 3000 + seed)
        one[len(one) // 2] = 0
        recs.append(one); kinds.append("single")
    while len(recs) < n_records(spec.M):
        recs.append(bases(n_bases(ls[int(rs.randint(0, len(ls)))]), 4000 + seed + len(recs))); kinds.append("filler")
    return recs, kinds


def _plant_sites(recs, W, rs):
    cdf = np.cumsum(synth.make_pwm(W, PWM_SEED).astype(np.float64), axis=0)
    for r in recs:
        site = (rs.random_sample(W)[None, :] > cdf[:3, :]).sum(axis=0).astype(np.uint8) + 1
        _plant(r, site, rs)


class FusedSet:
    """Records encoded by the oracle, the background learned from them, the seed model."""

    def __init__(self, orc, name, K, W, ss, records, kinds):
        self.name, self.K, self.W, self.ss, self.bg_order = name, K, W, ss, BG_ORDER
        self.records, self.kinds, self.N = records, kinds, len(records)
        in_off = np.concatenate([[0], np.cumsum([len(r) for r in records])]).astype(np.uint64)
        codes = np.concatenate(records)
        kinds_a = np.array(kinds)
        single = np.flatnonzero(kinds_a == "single")
        with_n = np.array([bool((r == 0).any()) for r in records])
        for self.encoder_seed in range(42, 106):             # an N is a random base per k-mer that covers it: libc's rand()
            _, self.kmer, self.off = orc.encode_set(codes, in_off, ss, self.encoder_seed)
            exc = kmer_exception_counts(self.kmer, self.off, K)
            # (at K = 0 an N is just its random base: no k-mer reaches back to it, no exception)
            if all(min(K, 1) <= exc[i] <= K + 2 for i in single) and (not ss or not exc[~with_n].any()):
                break
        else:
            raise AssertionError(f"{name}: no encoder seed gives the single N its exceptions")
        self.single = int(single[0]) if len(single) else None
        self.lens = np.diff(self.off.astype(np.int64))
        self.vbg = orc.bg_model(self.kmer, self.off, BG_ORDER, ALPHA_BG)
        self.A = synth.alpha_matrix(synth.default_alpha(K), W)
        pwm = synth.make_pwm(W, PWM_SEED)
        self.v0, self.q0 = synth.bamm_from_pwm(((1.0 - BLEND) * pwm + BLEND * 0.25).astype(np.float32), K), Q
        for a in (self.kmer, self.off, self.vbg, self.A, self.v0):
            a.setflags(write=False)

    def inputs(self, v=None, q=None, keep=None) -> regimes.Inputs:
        """regimes.Inputs of a model (the seed model by default) on the whole set, or on the records `keep` alone."""
        kmer, off = (self.kmer, self.off) if keep is None else subset(self.kmer, self.off, keep)
        case = SimpleNamespace(K=self.K, W=self.W, bg_order=self.bg_order, name=self.name)
        return regimes.Inputs(case, kmer, off, self.v0 if v is None else v, self.q0 if q is None else q, self.A, self.vbg)


_SETS: dict = {}


def case_set(orc, name: str) -> FusedSet:
    """The set of SPECS' case `name`: built once, shared, never modified."""
    if name not in _SETS:
        spec = SPEC_BY_NAME[name]
        seed = 37 * list(SPEC_BY_NAME).index(name)
        rs = np.random.RandomState(9000 + seed)
        recs, kinds = _records(spec, rs, seed)
        _plant_sites(recs, spec.W, rs)
        _SETS[name] = FusedSet(orc, name, spec.K, spec.W, spec.ss, recs, kinds)
    return _SETS[name]


# ---------------------------------------------------------------- sets of several launches --

# name: [(class, records)], K = 2, W = 20, both strands.  `scattered`: records of the class with N at n_frac = 0.01 (and one at
# a third of the record, so that none stays without), which k_em_seq takes.
MULTI = {
    "three_classes": dict(parts=[(5, 8), (7, 40), (20, 12)], scattered=(7, 6), mask=True),
    "classes_20_24": dict(parts=[(20, 10), (24, 10)], scattered=None, mask=False),
}
MULTI_K, MULTI_W = 2, 20


def multi_set(orc, name: str):
    """(FusedSet, class per record -- 0 for a scattered-N record --, fold mask or None)."""
    key = ("multi", name)
    if key not in _SETS:
        d = MULTI[name]
        rs = np.random.RandomState(9900 + len(name))
        recs, cls = [], []
        for M, count in d["parts"]:
            lo, hi = 32 * prev_class(M), 32 * M - 1          # bases: 64 prev + 1 .. 64 M - 1 positions
            for i in range(count):
                n = lo if i == 0 else hi if i == 1 else int(rs.randint(lo, hi + 1))
                recs.append(bases(n, 5000 + 100 * M + i)); cls.append(M)
        if d["scattered"]:
            M, count = d["scattered"]
            for i in range(count):
                r = bases(int(rs.randint(32 * prev_class(M) + 8, 32 * M)), 6000 + i)
                r[rs.random_sample(len(r)) < 0.01] = 0
                r[len(r) // 3] = 0
                recs.append(r); cls.append(0)
        order = rs.permutation(len(recs))
        recs, cls = [recs[i] for i in order], np.array(cls)[order]
        _plant_sites(recs, MULTI_W, rs)
        fs = FusedSet(orc, name, MULTI_K, MULTI_W, False, recs, ["filler"] * len(recs))
        mask = None
        if d["mask"]:
            mask = (np.arange(fs.N) % 3 != 0).astype(np.uint8)
            mask[-1] = 0
        _SETS[key] = (fs, cls, mask)
    return _SETS[key]


# ---------------------------------------------------------------------------- bars --

PAIR = "fused_classes"                                       # the `regime` under which regimes.PAIR_BARS would list a case


def bars(name: str, inp: regimes.Inputs) -> dict:
    """{quantity: (rtol, atol)} of the comparison with fp64: tests/regimes.py's bars as they stand, and twice the CPU test's
    figure where regimes.PAIR_BARS lists (PAIR, name, quantity) (the ratio atol / rtol kept, as regimes.v_bar keeps it)."""
    base = {"r": (regimes.R_RTOL * regimes.r_len_factor(inp.off), regimes.R_ATOL), "llh": (regimes.LLH_RTOL, regimes.llh_atol(inp.N)),
            "counts": (regimes.N_RTOL, regimes.N_ATOL), "v": (regimes.V_RTOL, regimes.V_ATOL)}
    out = {}
    for k, (rtol, atol) in base.items():
        wide = max(rtol, regimes.PAIR_BARS.get((PAIR, name, k), 0.0))
        out[k] = (wide, atol * (wide / rtol))
    return out
