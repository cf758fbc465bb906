"""k_score (csrc/scorer.hip; its chain is score_chain, which k_score_tile runs too) in every one of its 23 length
classes, with N exceptions under it: per class the shortest and the longest record it takes, N at the record's ends, around the first lane's last position and in a run across the
lane boundary in the middle of the wave; for three classes a record whose maxima tie across lanes.  mops, zoops and z
must be equal to the CPU oracle's element for element, with and without mops.  (test_logodds_bit_exact reaches the
classes up to 16 positions per lane and has no N in its long case; test_score_tiles_gpu.py covers the records beyond
8192 positions.)  Placements beyond a record's end are left out: the first class's shortest record (W positions, or 1)
has only the N that fit, its longest (64 positions) has them all, the run across lanes 31 | 32 included.  About 88 000
positions per call."""
import numpy as np
import pytest

import bammmotif2_amd as bm
from tests.test_score_tiles_gpu import Scored, bases

pytestmark = pytest.mark.gpu

M_CLASSES = [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32, 40, 48, 56, 64, 80, 96, 128]   # positions per lane
TIE_CLASSES = (7, 20, 64)


def with_n(L, M, K, seed):
    """L random bases; N (code 0) at 0, M - 1, M and L - 1 and a run of K + 2 across the lane boundary at 32 * M"""
    r = bases(L, seed)
    run = 32 * M - (K + 2) // 2
    for p in [0, M - 1, M, L - 1] + list(range(run, run + K + 2)):
        if 0 <= p < L:
            r[p] = 0
    return r


def class_records(K, W):
    """[(M, record)]: the shortest and the longest record of every class, then the tie records"""
    out, prev = [], 0
    for M in M_CLASSES:
        for L in (max(W, 64 * prev + 1), 64 * M):
            out.append((M, with_n(L, M, K, 1000 + 2 * len(out))))
        prev = M
    unit = bases(16, 7)
    for M in TIE_CLASSES:
        out.append((M, np.tile(unit, 4 * M)))             # 64 * M positions, the same 16 bases over and over
    return out


@pytest.mark.parametrize("K,W", [(2, 12), (0, 1)])
def test_every_class_with_exceptions(gpu_ctx, orc, K, W):
    recs = class_records(K, W)
    s = Scored(gpu_ctx, orc, [r for _, r in recs], True, K, W)
    try:
        assert np.array_equal(s.lens, [len(r) for _, r in recs])                  # single strand: as long as the input
        assert all(64 * (M_CLASSES[M_CLASSES.index(M) - 1] if M > 1 else 0) < len(r) <= 64 * M for M, r in recs)
        assert bm.score_plan(gpu_ctx, s.seqs, K, W)["wave_seqs"] == len(recs)     # every record goes through k_score
        mops, zoops, z = s.gpu(True)
        for name, g, o in zip(("mops", "zoops", "z"), (mops, zoops, z), s.oracle):
            bad = np.nonzero(g != o)[0]
            assert np.array_equal(g, o), f"{name} differs from the oracle at {bad[:8]} (of {len(bad)})"
        none, zoops2, z2 = s.gpu(True, want_mops=False)
        assert none is None and np.array_equal(zoops2, s.oracle[1]) and np.array_equal(z2, s.oracle[2])
        for n in range(len(recs) - len(TIE_CLASSES), len(recs)):                  # the tie records: the maximum is reached
            M = recs[n][0]                                                        # in more than one lane, the lowest window reported
            at = np.nonzero(s.oracle[0][s.moff[n]:s.moff[n + 1]] == s.oracle[1][n])[0]
            assert (at[-1] + W - 1) // M > (at[0] + W - 1) // M and z[n] == at[0]
    finally:
        s.close()
