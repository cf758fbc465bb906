"""Numerical regimes for the EM pass (helper; not collected by pytest).

tests/cases.py::Case feeds every kernel test one point in the space of numbers: a blurred PWM repeated at
every order, q = 0.3, an alpha that is constant over the columns, a background learned from uniform
sequences.  The builders here leave that point on purpose -- context-dependent and sharp models, exact
zeros, odds of exactly one, q and alpha at their ends, alpha that depends on the column, a wide dynamic
range -- over the same small shapes (FLAVOURS: one per kernel flavour).

inputs(orc, regime, flavour) returns the arrays in the ABI's layouts (include/bamm_em.h: v and A flat
[k][y][j] / [k][j], vbg flat [k][y]); reference() adds the fp64 expectations.  The builders draw integers
from numpy's frozen RandomState streams and only add, multiply and divide them: no libm call, so the
bytes are the same on every machine.

estep_f64 is a plain numpy fp64 restatement of one E step (EM.cpp:149-196, with the truncation of
EM.cpp:167): the oracle's em_step_f64 returns the model, the counts and the sums but not r itself.
"""
from __future__ import annotations

import numpy as np

from bammmotif2_amd import synth
from tests.cases import SMALL_CASES, Case

R_RTOL, R_ATOL = 2e-5, 1e-12          # tests/fuzz_parity.py's bar on r (W > 2), times r_len_factor()
V_RTOL, V_ATOL = 1e-6, 1e-9           # ... on the model after one step
N_RTOL, N_ATOL = 3e-6, 2e-7           # ... on the counts
LLH_RTOL = 2e-6                       # ... on the log-likelihood, with llh_atol()


# Where the CPU gate (tests/test_regimes_cpu.py) shows that the reference's own fp32 evaluation misses a bar, the bar of
# that pair is twice the gate's figure (the kernels make the same number of roundings in another order), never below the
# fuzz bar.  Only the pairs the kernels need are listed; the gate checks the figures.
#   alpha = 1e-3 at K = 4, W = 30: most contexts have counts far below alpha, so v = (n + A v') / (n' + A) is a ratio
#   of two small numbers and inherits the relative error of both
PAIR_BARS = {
    ("R7_alpha_1e-3", "k4", "v"): 2 * 1.257e-06,           # the gate measures 1.257e-06
    ("R6_alpha_alternating", "k4", "v"): 2 * 1.257e-06,    # the gate measures 1.257e-06 (the even columns have alpha = 1e-3)
    # tests/em_classes.py looks its pairs up here as ("em_classes_<flavour>_<model>", "<flavour><M>", quantity) -- any of r, llh,
    # counts, v -- and tests/test_em_classes_cpu.py holds an entry to twice its own figure.  None is listed: the restatement
    # misses bars under the blurred model in 31 (flavour, class) pairs from 8 positions per lane on (its sequential fp32 sums
    # over hundreds to thousands of windows: v 1.8e-5, counts 2.9e-5, llh 6.7e-6 on P128), the kernels, which do not sum that way,
    # keep the fuzz bars in every class (profiles/em_classes_margins.txt) -- so no bar is widened.
}


def v_bar(regime: str, shape: str):
    """(rtol, atol) on v: the figures above are max |a - b| / (|b| + atol / rtol) at the fuzz bar's atol / rtol, so a
    listed pair keeps that ratio -- the same measure, twice the threshold."""
    rtol = max(V_RTOL, PAIR_BARS.get((regime, shape, "v"), 0.0))
    return rtol, V_ATOL * (rtol / V_RTOL)


def llh_atol(n_seqs: int) -> float:
    return 1e-5 + 1e-7 * n_seqs


def r_len_factor(off) -> float:
    return max(1.0, 4e-4 * int(np.diff(np.asarray(off).astype(np.int64)).max()))


def v_offset(k: int, W: int) -> int:
    return W * ((4 ** (k + 1) - 4) // 3)


def bg_offset(k: int) -> int:
    return (4 ** (k + 1) - 4) // 3


# ---------------------------------------------------------------------------- shapes --

def _spec(specs, name):
    return dict(next(d for d in specs if d["name"] == name))


def _flavours():
    from tests.test_grouped_gpu import GROUPED_CASES
    from tests.test_mask_gpu import CASES as MASK_CASES
    g = lambda name: _spec(GROUPED_CASES, name)
    fl = {
        # name: (spec, tuning while the handle is created, what the planner must report)
        "per_column": (_spec(SMALL_CASES, "k1_heavyN"), dict(grouped=0), "per_column"),
        "grouped_6mer": (g("g_k2_ds_m7_N"), {}, "grouped"),
        "grouped_g5": (g("g_k0_ss"), {}, "grouped"),
        "grouped_k3_odd": (g("g_k3_ds_m5_odd"), {}, "grouped"),
        "mixed_a1": (g("g_mix_a1_m4"), dict(group_layout=8), "mixed"),
        "mixed_a2": (g("g_mix_a2_m5"), dict(group_layout=8), "mixed"),
        "mixed_w20": (g("g_k2_ds_m7_N"), dict(group_layout=8), "mixed"),
        "sliced": (dict(name="k4", N=60, L0=120, W=30, K=4, ss=True), {}, "sliced"),
        # both strands of 4050..4350 bases: 8101..8701 positions, on either side of the 8192 the register kernels hold
        "window_by_window": (dict(name="long", N=6, L0=4200, W=12, K=2, ragged=150), {}, "long"),
        "order_7": (_spec(MASK_CASES, "m_k7"), {}, "order_7"),
    }
    # the table layouts, on the shapes test_every_table_layout_matches_exact_arithmetic selects
    for layout in (0, 2, 3):
        for short, name in (("k2_ds_N", "g_k2_ds_m7_N"), ("k1_ss", "g_k1_ss_m4"), ("k0_ds_w2", "g_k0_ds_w2")):
            fl[f"layout{layout}_{short}"] = (g(name), dict(group_layout=layout), "grouped")
    return fl


_FLAVOURS = None


def flavours():
    global _FLAVOURS
    if _FLAVOURS is None:
        _FLAVOURS = _flavours()
    return _FLAVOURS


BASE_FLAVOURS = ["per_column", "grouped_6mer", "grouped_g5", "grouped_k3_odd", "mixed_a1", "mixed_a2", "sliced",
                 "window_by_window", "order_7"]
LAYOUT_FLAVOURS = [f"layout{l}_{s}" for l in (0, 2, 3) for s in ("k2_ds_N", "k1_ss", "k0_ds_w2")]
REGIMES = ["R1_context", "R2_sharp", "R3_zeros", "R4_odds_one", "R5_q_1e-6", "R5_q_0.999999", "R5_q_0",
           "R6_alpha_ramp", "R6_alpha_alternating", "R7_alpha_1e-3", "R7_alpha_1e6"]
R8 = "R8_wide_range"
R8_FLAVOURS = ["grouped_6mer", "mixed_w20", "layout0_k2_ds_N", "layout2_k2_ds_N", "layout3_k2_ds_N"]   # K = 2, W = 20


def pairs():
    """Every (regime, flavour) the GPU test runs and the CPU gate pins."""
    out = [(r, f) for r in REGIMES for f in BASE_FLAVOURS]
    out += [(r, f) for r in ("R1_context", "R2_sharp", "R3_zeros") for f in LAYOUT_FLAVOURS]
    out += [(R8, f) for f in R8_FLAVOURS]
    return out


UPDATE_REGIMES = [r for r in REGIMES if r.startswith(("R6", "R7"))]


# ---------------------------------------------------------------------------- builders --

class Inputs:
    """One (regime, shape): the encoded sequences and (v, q, A, vbg)."""

    def __init__(self, case, kmer, off, v, q, A, vbg, zero_seqs=()):
        self.case, self.kmer, self.off = case, kmer, off
        self.K, self.W, self.bg_order, self.N = case.K, case.W, case.bg_order, len(off) - 1
        self.v, self.A, self.vbg = (np.ascontiguousarray(x, np.float32) for x in (v, A, vbg))
        self.q = float(np.float32(q))
        self.zero_seqs = tuple(zero_seqs)          # R3: sequences whose every window meets a zero of v


def _normalised(w):
    """[..., 4] integer weights -> float32 distributions over the last axis."""
    w = w.astype(np.float64)
    return (w / w.sum(axis=-1, keepdims=True)).astype(np.float32)


def _flat_v(per_order, W):
    """per_order[k]: [4^k contexts][W][4 bases] -> flat [k][y = ctx * 4 + base][j]."""
    return np.ascontiguousarray(np.concatenate([p.transpose(0, 2, 1).reshape(-1, W).ravel() for p in per_order]), np.float32)


def context_model(K, W, seed):
    """R1: every order, context and column has a distribution of its own (squared integer weights 1..99: the smallest
    entry is about 3e-5, the largest about 0.99); a lower order is not a tiled copy of anything."""
    rs = np.random.RandomState(seed + 101)
    per_order = []
    for k in range(K + 1):
        w = rs.randint(1, 100, size=(4 ** k, W, 4)).astype(np.int64)
        per_order.append(_normalised(w * w))
    return _flat_v(per_order, W)


def zeroed_model(v0, K, W, seed):
    """R3: one base of every (order, context, column) set to exactly 0 and the other three renormalised -- a quarter of
    the cells.  Column 0 loses A and T in every context and column 1 loses T, so that a run of A (and its reverse
    strand, a run of T behind the junction's random base) meets a zero in every window."""
    rs = np.random.RandomState(seed + 303)
    out = []
    for k in range(K + 1):
        vk = v0[v_offset(k, W):v_offset(k + 1, W)].astype(np.float64).reshape(4 ** k, 4, W)
        drop = rs.randint(0, 4, size=(4 ** k, W))
        keep = np.ones(vk.shape, bool)                               # [context][base][column]
        keep[np.arange(4 ** k)[:, None], drop, np.arange(W)[None, :]] = False
        keep[:, :, 0] = True
        keep[:, [0, 3], 0] = False
        if W > 1:
            keep[:, :, 1] = True
            keep[:, 3, 1] = False
        vk = np.where(keep, vk, 0.0)
        vk /= vk.sum(axis=1, keepdims=True)
        out.append(vk.reshape(-1, W).ravel())
    return np.ascontiguousarray(np.concatenate(out), np.float32)


def wide_background():
    """R8: an order-2 background written by hand, conditional probabilities between 0.02 and 0.9, every context summing
    to one: flat [k][context * 4 + base]."""
    rows = np.array([[0.90, 0.02, 0.04, 0.04], [0.02, 0.90, 0.04, 0.04], [0.04, 0.04, 0.90, 0.02], [0.04, 0.04, 0.02, 0.90],
                     [0.40, 0.10, 0.10, 0.40], [0.10, 0.40, 0.40, 0.10], [0.25, 0.25, 0.25, 0.25], [0.02, 0.30, 0.60, 0.08]],
                    np.float64)
    order0 = np.array([0.30, 0.20, 0.20, 0.30])
    order1 = rows[[4, 5, 7, 6]]
    order2 = rows[[0, 5, 1, 6, 4, 2, 7, 3, 6, 0, 5, 1, 7, 4, 3, 2]]
    return np.concatenate([order0, order1.ravel(), order2.ravel()]).astype(np.float32)


def sharp_pwm(W, seed, squarings):
    """synth.make_pwm's integer weights (the same draws) raised to 2^squarings by repeated multiplication: at 3 it is
    make_pwm(W, seed, sharp=8), at 5 the largest base of a column holds more than 0.99 of it unless the two largest
    weights are within a seventh of each other."""
    rs = np.random.RandomState(seed)
    w = rs.randint(1, 100, size=(W, 4)).astype(np.float64)
    for _ in range(squarings):
        w = w * w
    cols = w / w.sum(axis=1, keepdims=True)
    cols = np.maximum(cols, 1e-4)
    cols /= cols.sum(axis=1, keepdims=True)
    return np.ascontiguousarray(cols.T.astype(np.float32))


# R2 is "one window per sequence carries r ~ 1": r = (q / LW1) odds / Z needs odds >> (1 - q) LW1 / q, and a window's
# odds cannot exceed about 4^W.  make_pwm(sharp=8) with q = 0.3 gets there at W = 20 only; the short motifs need a
# sharper matrix and a q near one (W = 7 on 95 windows: 4^7 = 16 384 against 99 * 0.7 * 95 / 0.3 = 21 945 for r = 0.99).
# (squarings, q) per shape; W = 2 (g_k0_ds_w2: odds <= 16 on 340 windows) cannot reach the regime at any q below
# 0.9995 and keeps the issue's parameters -- test_regimes_cpu.py asserts sharpness on every other shape.
R2_DEFAULT = (5, 0.3)
R2_SHAPES = {"k1_heavyN": (7, 0.99), "m_k7": (7, 0.99), "long": (7, 0.3), "g_k0_ds_w2": (3, 0.3)}
R2_NOT_SHARP = ("g_k0_ds_w2",)


def _sharp_case(spec, sharp=None, squarings=None):
    """The shape's sequences with a site of a sharp PWM planted in every one of them."""
    c = Case(**spec)
    c.pwm = synth.make_pwm(c.W, c.seed, sharp=sharp) if squarings is None else sharp_pwm(c.W, c.seed, squarings)
    c.codes, c.in_off = synth.make_sequences(c.N, c.L0, c.pwm, c.seed, 1.0, c.n_frac, c.ragged)
    return c


R8_SHARP, R8_BLUR = 8, 0.02            # chosen on the CPU so that the gate's two range conditions hold (test_regimes_cpu.py)


def inputs(orc, regime, flavour) -> Inputs:
    spec = dict(flavours()[flavour][0])
    zero_seqs = ()
    if regime == "R2_sharp":
        c = _sharp_case(spec, squarings=R2_SHAPES.get(spec["name"], R2_DEFAULT)[0])
    elif regime == R8:
        c = _sharp_case(spec, R8_SHARP)
    else:
        c = Case(**spec)
    if regime == "R3_zeros":                     # three runs of A (code 1), in the first, a middle and the last block's reach
        lens = np.diff(c.in_off.astype(np.int64))
        zero_seqs = (1, c.N // 2, c.N - 1)
        for n in zero_seqs:
            c.codes[int(c.in_off[n]):int(c.in_off[n]) + int(lens[n])] = 1
    _, kmer, off, vbg = c.encode(orc)
    v, q, A = c.v0, c.q, c.A
    K, W = c.K, c.W
    if regime == "R1_context":
        v = context_model(K, W, c.seed)
    elif regime == "R2_sharp":
        v = synth.bamm_from_pwm(c.pwm, K)
        q = R2_SHAPES.get(c.name, R2_DEFAULT)[1]
    elif regime == "R3_zeros":
        v = zeroed_model(c.v0, K, W, c.seed)
    elif regime == "R4_odds_one":
        v = np.full_like(c.v0, 0.25)
        vbg = np.full_like(vbg, 0.25)
    elif regime.startswith("R5_q_"):
        q = float(regime[len("R5_q_"):])
    elif regime == "R6_alpha_ramp":
        A = (c.alpha.astype(np.float64)[:, None] * (1 + np.arange(W))[None, :]).astype(np.float32).ravel()
    elif regime == "R6_alpha_alternating":
        A = np.tile(np.where(np.arange(W) % 2 == 0, 1e-3, 1e4), K + 1).astype(np.float32)
    elif regime == "R7_alpha_1e-3":
        A = np.full((K + 1) * W, 1e-3, np.float32)
    elif regime == "R7_alpha_1e6":
        A = np.full((K + 1) * W, 1e6, np.float32)
    elif regime == R8:
        assert K == 2 and c.bg_order == 2 and W >= 20
        vbg = wide_background()
        v = synth.bamm_from_pwm(((1.0 - R8_BLUR) * c.pwm.astype(np.float64) + R8_BLUR * 0.25).astype(np.float32), K)
    return Inputs(c, kmer, off, v, q, A, vbg, zero_seqs)


# ---------------------------------------------------------------------------- fp64 E step --

def odds_f64(inp: Inputs):
    """[4^(K+1)][W] fp64 odds v[K] / vbg[min(bg_order, K)] (Motif.cpp:485-494)."""
    K, W = inp.K, inp.W
    Y, Kb = 4 ** (K + 1), min(inp.bg_order, inp.K)
    vK = inp.v[v_offset(K, W):v_offset(K + 1, W)].astype(np.float64).reshape(Y, W)
    b = inp.vbg[bg_offset(Kb):bg_offset(Kb + 1)].astype(np.float64)
    return vK / b[np.arange(Y) % 4 ** (Kb + 1)][:, None]


def window_products(s, y, W, LW1):
    """p[i] = prod_j s[y[i + j]][j] over the columns with i + j < LW1 (EM.cpp:167: the last W - 1 windows are cut)."""
    p = np.ones(LW1, np.float64)
    for j in range(min(W, LW1)):
        m = LW1 - j
        p[:m] *= s[y[j:j + m], j]
    return p


def estep_f64(inp: Inputs):
    """One E step in fp64: (r in getR()'s layout -- window start i of a sequence of L positions at L - W - i, the last
    W - 1 slots zero --, Z per sequence, llh = sum log Z, sum of r, counts flat [k][y][j] rebuilt from r)."""
    K, W, q = inp.K, inp.W, inp.q
    Y = 4 ** (K + 1)
    s = odds_f64(inp)
    off = inp.off.astype(np.int64)
    r = np.zeros(int(off[-1]), np.float64)
    Z = np.zeros(inp.N, np.float64)
    nK = np.zeros((Y, W), np.float64)
    sum_r = 0.0
    for n in range(inp.N):
        o, L = int(off[n]), int(off[n + 1] - off[n])
        LW1 = L - W + 1
        y = (inp.kmer[o:o + LW1] % np.uint64(Y)).astype(np.int64)
        rw = window_products(s, y, W, LW1) * q / LW1
        Z[n] = (1.0 - q) + rw.sum()
        rw = rw / Z[n]
        r[o:o + LW1] = rw[::-1]
        sum_r += rw.sum()
        for j in range(min(W, LW1)):                      # EM.cpp:230-243: position ij, column j <- window ij - j
            np.add.at(nK[:, j], y[j:], rw[:LW1 - j])
    counts = [nK]
    for k in range(K, 0, -1):                             # EM.cpp:247-254
        counts.insert(0, counts[0].reshape(4, 4 ** k, W).sum(axis=0))
    return r, Z, float(np.log(Z).sum()), float(sum_r), np.concatenate([c.ravel() for c in counts])


def odds_one_closed_form(inp: Inputs):
    """R4 (every odds value exactly 1): r = (q / LW1) / Z with Z = 1 - q + LW1 * (q / LW1), llh = sum log Z, and the
    order-K counts are r times the number of positions that carry the k-mer."""
    K, W, q = inp.K, inp.W, inp.q
    Y = 4 ** (K + 1)
    off = inp.off.astype(np.int64)
    r = np.zeros(int(off[-1]), np.float64)
    nK = np.zeros((Y, W), np.float64)
    llh = 0.0
    for n in range(inp.N):
        o, L = int(off[n]), int(off[n + 1] - off[n])
        LW1 = L - W + 1
        Z = (1.0 - q) + LW1 * (q / LW1)
        r[o:o + LW1] = (q / LW1) / Z
        llh += float(np.log(Z))
        y = (inp.kmer[o:o + LW1] % np.uint64(Y)).astype(np.int64)
        for j in range(min(W, LW1)):
            nK[:, j] += np.bincount(y[j:], minlength=Y) * ((q / LW1) / Z)
    return r, llh, nK


class Reference:
    """What one (regime, shape) must give: computed once, shared by the tests that need it, never modified."""

    def __init__(self, orc, inp: Inputs):
        self.r64, self.Z, self.llh_np, self.sum_r_np, self.n_np = estep_f64(inp)
        self.v64, self.n64, self.llh64, self.sum_r64 = orc.em_step_f64(inp.kmer, inp.off, inp.K, inp.W, inp.bg_order, inp.vbg,
                                                                       inp.A, inp.v, inp.q)
        # the fp32 restatement of the reference (sequential sums, left-to-right products)
        Kb = min(inp.bg_order, inp.K)
        self.s32 = orc.linear_s(inp.v, inp.vbg, inp.K, inp.W, Kb)
        self.r32, self.llh32 = orc.estep(inp.kmer, inp.off, inp.K, inp.W, self.s32, inp.q)
        for a in (self.r64, self.Z, self.n_np, self.v64, self.n64, self.r32):
            a.setflags(write=False)


_CACHE: dict = {}


def case(orc, regime, flavour):
    """(Inputs, Reference) of a pair; layouts and tunings of one shape share the entry."""
    spec_name = flavours()[flavour][0]["name"]
    key = (regime, spec_name)
    if key not in _CACHE:
        inp = inputs(orc, regime, flavour)
        _CACHE[key] = (inp, Reference(orc, inp))
    return _CACHE[key]
