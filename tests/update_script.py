"""The model update and optimize()'s loop as a pure function of a script (helper; not collected by pytest).

EM.set_allreduce(fn) is called with (dev_ptr, n_words, stream) between the local accumulation and the update of every
pass of iterate(), optimize() and MStep() -- fused handles included, where it receives the ring slot the pass just added
into.  Scripted installs a callback that OVERWRITES those words with integers the test chose: the real kernels still run
(they carry the fused prologue and the stop flag), their sums are replaced, and what the update must give is
expected_update(): a plain numpy / oracle restatement of EM.cpp:247-254, Motif.h:95-136 (orc.update_v), Motif.cpp:485-494
(orc.linear_s), EM.cpp:515 and EM.cpp:102-108 on the same integers.

The accumulator's layout (csrc/common.h, UpdateArgs::acc): the order-K counts [y][j] in units of 2^-shift, then three
words -- llh in units of 2^-24, the sum of r in units of 2^-30, the sequence count in the low 40 bits of the third with a
count of blocks whose statistics were not finite from bit 40 up (csrc/device_utils.h).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

LLH_UNIT, SUMR_UNIT, BAD_UNIT = 1 << 24, 1 << 30, 1 << 40


def v_offset(k: int, W: int) -> int:
    return W * ((4 ** (k + 1) - 4) // 3)


def cells_of(K: int, W: int) -> int:
    return 4 ** (K + 1) * W


# ---------------------------------------------------------------------------- the expectation --

def marginalise(nK: np.ndarray, K: int, W: int) -> np.ndarray:
    """float32 [4^(K+1)][W] -> flat [k][y][j] over every order: n[k-1][y2][j] = (((0 + c0) + c1) + c2) + c3 over the four
    rows y = d * 4^k + y2 of order k, ascending, in float32 (EM.cpp:247-254: `+=` into a zeroed cell, y ascending)."""
    tabs = [np.ascontiguousarray(nK, np.float32).reshape(4 ** (K + 1), W)]
    for k in range(K, 0, -1):
        src = tabs[0].reshape(4, 4 ** k, W)
        acc = np.zeros((4 ** k, W), np.float32)
        for d in range(4):
            acc = (acc + src[d]).astype(np.float32)
        tabs.insert(0, acc)
    return np.concatenate([t.ravel() for t in tabs])


def decode_stats(words):
    """(llh, sum_r, nseq) in fp64 from the three statistics words; llh is NaN when any bit from 40 up of the third is set."""
    x0, x1, x2 = (int(w) for w in words)
    llh = float("nan") if (x2 >> 40) != 0 else x0 / LLH_UNIT
    return llh, x1 / SUMR_UNIT, float(x2 & (BAD_UNIT - 1))


def expected_update(acc_words, shift, K, W, Kbg, A, vbg, v_old, q_in, optimize_q, n_seqs_global, orc):
    """(n, v, s, q, llh, sum_r, nseq, v_diff64) of one update: n, v flat [k][y][j] and s [y][j] in float32 (bit for bit what
    the device must hold), q the fp64 value of EM.cpp:515 (q_in outside the window), llh / sum_r / nseq fp64 as decoded,
    v_diff64 = fsum |float32(v - v_old)| over the top order."""
    acc = np.asarray(acc_words, np.int64)
    cells = cells_of(K, W)
    assert acc.size == cells + 3
    nK = (acc[:cells].astype(np.float64) * 2.0 ** -shift).astype(np.float32)
    n = marginalise(nK, K, W)
    A, vbg = np.ascontiguousarray(A, np.float32), np.ascontiguousarray(vbg, np.float32)
    v = orc.update_v(n, A, vbg, K, W)
    s = orc.linear_s(v, vbg, K, W, Kbg)
    llh, sum_r, nseq = decode_stats(acc[cells:])
    if n_seqs_global:
        nseq = float(n_seqs_global)
    q = (nseq - sum_r + 1.0) / (nseq + 2.0) if optimize_q else float(q_in)
    top = slice(v_offset(K, W), v_offset(K + 1, W))
    d32 = np.abs((v[top] - np.ascontiguousarray(v_old, np.float32)[top]).astype(np.float32))
    return n, v, s, q, llh, sum_r, nseq, math.fsum(d32.astype(np.float64).tolist())


def far_from_a_tie(x64: float, rel=1e-9) -> bool:
    """x64 lies farther than `rel` (relative) from the midpoint of the two float32 values around it: whatever the grouping
    of an fp64 sum (errors of some cells * 2^-53), it rounds to the same float32."""
    f = np.float32(x64)
    if float(f) == x64 or x64 == 0.0:
        return True
    other = np.nextafter(f, np.float32(np.inf) if float(f) < x64 else np.float32(-np.inf))
    mid = 0.5 * (float(f) + float(other))
    return abs(x64 - mid) > rel * abs(x64)


# ---------------------------------------------------------------------------- scripts --

def stats(llh=0.0, sum_r=0.0, nseq=0, bad=0):
    """The three statistics words for llh (a multiple of 2^-24), sum_r (of 2^-30), nseq sequences and `bad` flagged blocks."""
    x0, x1 = llh * LLH_UNIT, sum_r * SUMR_UNIT
    assert x0 == int(x0) and x1 == int(x1) and 0 <= nseq < BAD_UNIT
    return [int(x0), int(x1), int(nseq) + int(bad) * BAD_UNIT]


def row(counts, st):
    return np.concatenate([np.asarray(counts, np.int64), np.asarray(st, np.int64)])


def counts_random(rs, K, W):
    """ints below 2^50, 30 % exact zeros"""
    c = rs.randint(0, 1 << 50, size=cells_of(K, W), dtype=np.int64)
    c[rs.random_sample(c.size) < 0.3] = 0
    return c


def counts_zero(rs, K, W):
    """nothing was counted: the update walks the prior chain alone"""
    return np.zeros(cells_of(K, W), np.int64)


def counts_sparse(rs, K, W):
    """one non-zero cell per column"""
    c = np.zeros((4 ** (K + 1), W), np.int64)
    c[rs.randint(0, 4 ** (K + 1), size=W), np.arange(W)] = rs.randint(1, 1 << 50, size=W, dtype=np.int64)
    return c.ravel()


def counts_wide(rs, K, W):
    """a few cells near 2^61 beside cells holding one unit"""
    c = np.ones(cells_of(K, W), np.int64)
    big = rs.choice(c.size, size=min(c.size, 3), replace=False)
    c[big] = (1 << 61) - rs.randint(0, 1 << 20, size=big.size, dtype=np.int64)
    return c


COUNTS = dict(random=counts_random, zero=counts_zero, sparse=counts_sparse, wide=counts_wide)


def random_stats(rs, nseq):
    """llh of either sign, sum_r between 0 and nseq"""
    return stats(int(rs.randint(-(1 << 30), 1 << 30)) / LLH_UNIT, int(rs.randint(0, max(nseq, 1) << 30)) / SUMR_UNIT, nseq)


def script(kind, seed, K, W, n_rows, nseq):
    rs = np.random.RandomState(seed)
    return [row(COUNTS[kind](rs, K, W), random_stats(rs, nseq)) for _ in range(n_rows)]


# ---------------------------------------------------------------------------- the device side --

_HIP = None
D2H, H2D, D2D = 2, 1, 3


def hip():
    global _HIP
    if _HIP is None:
        _HIP = C.CDLL("libamdhip64.so")
        _HIP.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _HIP.hipFree.argtypes = [C.c_void_p]
        _HIP.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _HIP.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return _HIP


def poke(ctx, em, words):
    """The words of the handle's accumulator overwritten, for the hand-driven accumulate() / update() pair (which calls no
    all-reduce: the caller sums the buffer it asked for)."""
    ctx.sync()
    p, n = em.reduce_buffer()
    w = np.ascontiguousarray(words, np.int64)
    assert n == w.size
    assert hip().hipMemcpy(C.c_void_p(p), w.ctypes.data_as(C.c_void_p), n * 8, H2D) == 0


def peek(ctx, em):
    ctx.sync()
    p, n = em.reduce_buffer()
    w = np.zeros(n, np.int64)
    assert hip().hipMemcpy(w.ctypes.data_as(C.c_void_p), C.c_void_p(p), n * 8, D2H) == 0
    return w


class Scripted:
    """rows[c] replaces the sums of the handle's c-th all-reduce from now on; calls beyond the last row leave the words
    alone (optimize()'s look-ahead units behind a raised flag, where a real all-reduce would sum untouched zeros)."""

    def __init__(self, ctx, em, rows):
        self.em, self.calls = em, 0
        self.rows = np.ascontiguousarray(np.stack(rows), np.int64)
        self.n_words = self.rows.shape[1]
        assert self.n_words == cells_of(em.K, em.W) + 3
        self.block = C.c_void_p()
        assert hip().hipMalloc(C.byref(self.block), self.rows.nbytes) == 0
        assert hip().hipMemcpy(self.block, self.rows.ctypes.data_as(C.c_void_p), self.rows.nbytes, H2D) == 0
        em.set_allreduce(self._call)

    def _call(self, dev_ptr, n_words, stream):
        assert n_words == self.n_words, (n_words, self.n_words)
        c = self.calls
        self.calls += 1
        if c >= len(self.rows):
            return 0
        src = C.c_void_p(self.block.value + c * self.n_words * 8)
        return hip().hipMemcpyAsync(C.c_void_p(dev_ptr), src, self.n_words * 8, D2D, C.c_void_p(stream or None))

    def close(self, ctx):
        """The callback removed and the block freed (after whatever still reads it has run)."""
        self.em.set_allreduce(None)
        ctx.sync()
        if self.block:
            hip().hipFree(self.block)
            self.block = C.c_void_p()


# ---------------------------------------------------------------------------- handles --

TUNING_DEFAULTS = dict(group_layout=-1, grouped=1, update_blocks=1, fused_update=1)
LDS, ONE_BLOCK, BANDS = 0, 1, 2                               # EM.plan_update()'s forms
ALPHA_REGIMES = ("R6_alpha_ramp", "R7_alpha_1e-3", "R7_alpha_1e6")
_INPUTS: dict = {}


def alpha_of(regime, alpha, K, W):
    """A[k][j] of tests/regimes.py's alpha regimes on any shape (regimes.inputs builds them per flavour)."""
    if regime == "R6_alpha_ramp":
        return (alpha.astype(np.float64)[:, None] * (1 + np.arange(W))[None, :]).astype(np.float32).ravel()
    return np.full((K + 1) * W, {"R7_alpha_1e-3": 1e-3, "R7_alpha_1e6": 1e6}[regime], np.float32)


def tiny_inputs(orc, K, W, N=16, regime=None):
    """regimes.Inputs of N short sequences for a (K, W) no flavour has: they only carry the launch."""
    from tests import regimes
    from tests.cases import Case
    key = (K, W, N, regime)
    if key not in _INPUTS:
        c = Case(f"u_k{K}_w{W}", N, max(40, W + 10), W, K)
        _, kmer, off, vbg = c.encode(orc)
        A = c.A if regime is None else alpha_of(regime, c.alpha, K, W)
        _INPUTS[key] = regimes.Inputs(c, kmer, off, c.v0, c.q, A, vbg)
    return _INPUTS[key]


def flavour_inputs(orc, flavour, regime="base"):
    """regimes.Inputs of a flavour's shape; "base" (no regime of that name: every branch of regimes.inputs passes) is
    tests/cases.py's own point."""
    from tests import regimes
    key = (flavour, regime)
    if key not in _INPUTS:
        _INPUTS[key] = regimes.inputs(orc, regime, flavour)
    return _INPUTS[key]


def open_tiny(ctx, inp, tuning, v=None, q=None, **kw):
    """(em, seqs) over inp's sequences, created under `tuning` (restored afterwards)."""
    import bammmotif2_amd as bm
    ss = bm.SeqSet(ctx, bm.PackedSeqs.from_kmers(inp.kmer, inp.off))
    ctx.set_tuning(**tuning)
    try:
        em = bm.EM(ctx, ss, inp.K, inp.W, inp.vbg, inp.A, inp.v if v is None else v, inp.q if q is None else q,
                   bg_order=inp.bg_order, **kw)
    finally:
        ctx.set_tuning(**{k: TUNING_DEFAULTS[k] for k in tuning})
    return em, ss


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_float(a, b) -> bool:
    """equal as float32, NaN equal to NaN"""
    return bool(np.array_equal(np.asarray([a], np.float32), np.asarray([b], np.float32), equal_nan=True))


def vdiff_ok(dev, d64) -> bool:
    """within one float32 ulp (2^-23 relative) of the fsum: the device's fp64 grouping differs from it by about
    cells * 2^-53, the ulp covers the final rounding"""
    return abs(float(dev) - d64) <= 2.0 ** -23 * d64


def q_ok(dev, q64) -> bool:
    """within 2^-22 absolute of the fp64 value of EM.cpp:515 (the reference's fp32 expression has four roundings of
    quantities <= N + 2 before and in the division by N + 2)"""
    return abs(float(dev) - q64) <= 2.0 ** -22


# ---------------------------------------------------------------------------- optimize()'s loop --

# kind: (how the handle is opened, what plan_update() must report); seeds chosen so that knife_edge()'s conditions hold
# (tests/test_update_script_cpu.py asserts them)
LOOP_KINDS = {
    "plain": dict(flavour="per_column", form=LDS, fusable=False, seed=11),
    "fused_mixed": dict(flavour="mixed_w20", form=LDS, fusable=True, seed=12),
    "fused_grouped": dict(flavour="grouped_6mer", form=LDS, fusable=True, seed=13),
    "bands": dict(shape=(3, 9), tuning=dict(update_blocks=1), form=BANDS, fusable=False, seed=14),
}


def loop_inputs(orc, kind):
    d = LOOP_KINDS[kind]
    return flavour_inputs(orc, d["flavour"]) if "flavour" in d else tiny_inputs(orc, *d["shape"])


def two_rows(kind, inp):
    """the two `random` count rows the loop scripts repeat or alternate: the second is the first with one cell in sixteen
    drawn again, so that a pass between them moves the model by far less (D) than the first pass moves the handle's initial
    model (D1) and an epsilon beside D cannot stop pass 1"""
    rs = np.random.RandomState(LOOP_KINDS[kind]["seed"])
    c0 = counts_random(rs, inp.K, inp.W)
    c1 = c0.copy()
    again = rs.choice(c0.size, size=max(4, c0.size // 16), replace=False)
    c1[again] = counts_random(rs, inp.K, inp.W)[again]
    return c0, c1


def knife_edge(orc, kind):
    """(D1, D): fp64 v_diff of the first pass (row 0 against the handle's initial model) and of every later pass of a
    script that alternates the two rows.  v after a pass is a function of that pass's counts alone."""
    inp = loop_inputs(orc, kind)
    Kbg = min(inp.bg_order, inp.K)
    c0, c1 = two_rows(kind, inp)
    e0 = expected_update(row(c0, stats(nseq=inp.N)), 40, inp.K, inp.W, Kbg, inp.A, inp.vbg, inp.v, inp.q, False, 0, orc)
    e1 = expected_update(row(c1, stats(nseq=inp.N)), 40, inp.K, inp.W, Kbg, inp.A, inp.vbg, e0[1], inp.q, False, 0, orc)
    e2 = expected_update(row(c0, stats(nseq=inp.N)), 40, inp.K, inp.W, Kbg, inp.A, inp.vbg, e1[1], inp.q, False, 0, orc)
    assert e2[7] == e1[7]                                    # |a - b| = |b - a| cell by cell
    return e0[7], e1[7]


def loop_rows(counts, llh, sum_r, nseq, bad=()):
    """one row per pass: counts[p mod len(counts)], llh[p], sum_r[p]; passes (1-based) in `bad` carry the non-finite flag"""
    return [row(counts[p % len(counts)], stats(llh[p], sum_r[p], nseq, 1 if p + 1 in bad else 0)) for p in range(len(llh))]
