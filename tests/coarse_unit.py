"""Coarse accumulator units (helper; not collected by pytest).

The counts of a pass travel as int64 fixed point in units of 2^-fix_shift: 40 up to 2^22 sequences, coarser beyond,
down to 24, sized from bamm_em_params.n_seqs_bound (csrc/em.cpp, bamm_em_create).  Two handles on the same set under the
same forced tuning, one at 40 and one at s < 40, d = 40 - s:

  per window   the scale is a power of two applied to 1/Z or to r, so the scaled fp32 value is the unscaled one times
               2^-d bit for bit, and the conversion truncates: F_s = F_40 >> d, exactly;
  per cell     a sum of floors is not the floor of the sum: 0 <= (acc_40[c] >> d) - acc_s[c] <= m_c, with m_c the
               number of addends of the cell (addend_bound) -- derived, nothing measured;
  statistics   llh (2^-24), sum of r (2^-30) and the sequence count do not depend on the unit: equal word for word.

Against fp64 the truncation can only lower a count, by less than one unit per addend: count_bar is the fuzz bar on
counts (regimes.N_RTOL / N_ATOL) with m * 2^-s more room on the low side.
"""
from __future__ import annotations

import numpy as np

from tests import regimes

# the smallest n_seqs_bound that gives the unit: fix_shift = min(40, 62 - min(ceil(log2(bound)), 38))
BOUNDS = {39: 1 << 23, 33: 1 << 29, 32: 1 << 30, 31: 1 << 31, 24: 1 << 38}


def fix_shift_of(bound: int) -> int:
    """The formula of bamm_em_create, restated: the int64 total of `bound` addends below 2^shift stays below 2^62."""
    bits = 0
    while (1 << bits) < max(bound, 1) and bits < 63:
        bits += 1
    return min(40, 62 - min(bits, 38))


def _windows(inp):
    """(o, LW1, y[LW1]) per sequence: y the order-K code of every position that a window may cover (EM.cpp:167 cuts the
    last W - 1 positions)."""
    Y = 4 ** (inp.K + 1)
    off = inp.off.astype(np.int64)
    for n in range(inp.N):
        o, L = int(off[n]), int(off[n + 1] - off[n])
        LW1 = L - inp.W + 1
        yield o, LW1, (inp.kmer[o:o + LW1] % np.uint64(Y)).astype(np.int64)


def addend_bound(inp) -> np.ndarray:
    """m[Y][W] (int64): the number of (sequence, window) pairs whose window puts a position with code y under column j --
    an upper bound on the number of addends of the accumulator's cell (y, j), whatever r is."""
    Y, W = 4 ** (inp.K + 1), inp.W
    m = np.zeros((Y, W), np.int64)
    for _, LW1, y in _windows(inp):
        for j in range(min(W, LW1)):
            m[:, j] += np.bincount(y[j:], minlength=Y)
    return m


def largest_addend(inp, r64: np.ndarray) -> np.ndarray:
    """[Y][W] (fp64): the largest r among the addends of every cell (0 where it has none), r in getR()'s layout.  A cell
    with an addend of r >= 2^-s cannot be empty at the unit 2^-s."""
    Y, W = 4 ** (inp.K + 1), inp.W
    top = np.zeros((Y, W), np.float64)
    for o, LW1, y in _windows(inp):
        rw = r64[o:o + LW1][::-1]
        for j in range(min(W, LW1)):
            np.maximum.at(top[:, j], y[j:], rw[:LW1 - j])
    return top


def all_orders(inp, top: np.ndarray) -> np.ndarray:
    """[Y][W] of order K -> flat [k][y][j] over every order, the lower ones summed as EM.cpp:247-254 sums the counts."""
    tabs = [top]
    for k in range(inp.K, 0, -1):
        tabs.insert(0, tabs[0].reshape(4, 4 ** k, inp.W).sum(axis=0))
    return np.concatenate([t.ravel() for t in tabs])


def windows_r(inp, r64: np.ndarray) -> np.ndarray:
    """r of every window that exists (getR()'s layout holds W - 1 empty slots per sequence), in one array."""
    return np.concatenate([r64[o:o + LW1] for o, LW1, _ in _windows(inp)])


def counts_from_r(inp, r64: np.ndarray, per_window=lambda r: r) -> np.ndarray:
    """Counts flat [k][y][j] (fp64) rebuilt from r in getR()'s layout, per_window applied to every window's r first."""
    Y, W = 4 ** (inp.K + 1), inp.W
    nK = np.zeros((Y, W), np.float64)
    for o, LW1, y in _windows(inp):
        rw = per_window(r64[o:o + LW1][::-1])
        for j in range(min(W, LW1)):
            np.add.at(nK[:, j], y[j:], rw[:LW1 - j])
    return all_orders(inp, nK)


def truncate(s: int):
    """r -> floor(r * 2^s) * 2^-s: what one window adds at the unit 2^-s (exact in fp64 for r <= 1, s <= 40)."""
    return lambda r: np.floor(np.ldexp(r, s)) * 2.0 ** -s


def applied_twice(s: int):
    """The deliberate mistake of the CPU gate: the scale 2^(s-40) applied twice in a threshold r * scale >= 2^-40 drops
    every window with r < 2^-(2s - 40); the others are truncated as usual."""
    cut = 2.0 ** -(2 * s - 40)
    return lambda r: np.where(r < cut, 0.0, truncate(s)(r))


def count_bar(n64: np.ndarray, m: np.ndarray, s: int):
    """(lo, hi) per cell of counts flat [k][y][j]: the fuzz bar around n64, widened by m * 2^-s on the low side only
    (truncation never raises a count).  m: addend_bound through all_orders."""
    n64 = np.asarray(n64, np.float64)
    tol = regimes.N_ATOL + regimes.N_RTOL * np.abs(n64)
    return n64 - tol - np.asarray(m, np.float64) * 2.0 ** -s, n64 + tol


def inside(counts, n64, m, s) -> np.ndarray:
    lo, hi = count_bar(n64, m, s)
    counts = np.asarray(counts, np.float64)
    return (counts >= lo) & (counts <= hi)


def fold_low_side(counts, n64, m, s) -> np.ndarray:
    """counts with the deficit that count_bar's widening allows taken out, so that the symmetric
    margins.check(fold_low_side(...), n64, N_RTOL, N_ATOL) is exactly `lo <= counts <= hi` of count_bar."""
    counts, n64 = np.asarray(counts, np.float64), np.asarray(n64, np.float64)
    return counts + np.clip(n64 - counts, 0.0, np.asarray(m, np.float64) * 2.0 ** -s)


def update_v_f64(inp, counts: np.ndarray) -> np.ndarray:
    """The model update in fp64 from given counts flat [k][y][j], every order as given (EM.cpp:256 -> Motif.h:95-136):
    v[0][y][j] = (n[0][y][j] + A[0][j] vbg[y]) / (sum_y n[0][y][j] + A[0][j]);
    v[k][y][j] = (n[k][y][j] + A[k][j] v[k-1][y mod 4^k][j]) / (n[k-1][y div 4][j-1] + A[k][j]) for j >= k, and
    v[k][y][j] = v[k-1][y mod 4^k][j] for the columns j < k, whose context would begin in front of the motif."""
    K, W = inp.K, inp.W
    n = np.asarray(counts, np.float64)
    A = inp.A.astype(np.float64).reshape(K + 1, W)
    n_of = lambda k: n[regimes.v_offset(k, W):regimes.v_offset(k + 1, W)].reshape(4 ** (k + 1), W)
    n0 = n_of(0)
    prev = (n0 + A[0][None, :] * inp.vbg[:4].astype(np.float64)[:, None]) / (n0.sum(axis=0)[None, :] + A[0][None, :])
    out = [prev]
    for k in range(1, K + 1):
        y = np.arange(4 ** (k + 1))
        lower = prev[y % 4 ** k]
        vk = lower.copy()
        denom = n_of(k - 1)[y // 4][:, k - 1:W - 1] + A[k][None, k:]
        vk[:, k:] = (n_of(k)[:, k:] + A[k][None, k:] * lower[:, k:]) / denom
        out.append(vk)
        prev = vk
    return np.concatenate([t.ravel() for t in out])
