"""Window p-values on the device, the parts that need no GPU: the C ABI declares and binds bamm_occurrences and its
accessors, the per-window formula the host and the device path share (csrc/occ_pvalue.h) gives the reference's p-values
(tests/golden/eval_small.npz, produced by ScoreSeqSet.cpp:70-126) when it is fed ranks and neighbours computed in numpy,
and the writer that takes a hit list reproduces the reference's .occurrence file (ScoreSeqSet.cpp:245-291)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bammmotif2_amd import abi, build
from tests import golden_util as gu

OCC_SYMBOLS = {"bamm_occurrences": 10, "bamm_occ_info": 7, "bamm_occ_get": 8, "bamm_occ_destroy": 1}


@pytest.fixture(scope="module")
def host(lib):
    build.build_host()
    H = C.CDLL(build.HOST_LIB)
    H.bh_last_error.restype = C.c_char_p
    return H


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(gu.GOLDEN_DIR, "eval_small.npz")))


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def ranks_and_neighbours(pos, neg_sorted):
    """FPl, SlHigher = neg[negN - FPl - 1], SlLower = neg[negN - FPl] as ScoreSeqSet.cpp:100-121 reads them (0 where the
    index does not exist; the formula does not look at them there)."""
    negN = len(neg_sorted)
    fp = (negN - np.searchsorted(neg_sorted, pos, side="right")).astype(np.uint64)     # std::upper_bound
    hi_idx, lo_idx = negN - fp.astype(np.int64) - 1, negN - fp.astype(np.int64)
    higher = np.where(hi_idx >= 0, neg_sorted[np.clip(hi_idx, 0, negN - 1)], 0).astype(np.float32)
    lower = np.where(lo_idx < negN, neg_sorted[np.clip(lo_idx, 0, negN - 1)], np.inf).astype(np.float32)
    return fp, higher, lower


def test_header_declares_and_abi_binds_the_occurrence_entry_points(lib):
    hdr = open(os.path.join(os.path.dirname(abi.HERE), "include", "bamm_em.h")).read()
    for name, n_args in OCC_SYMBOLS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/bamm_em.h"
        assert len(m.group(1).split(",")) == n_args, name
        assert name in abi.SYMBOLS
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == n_args, name
    assert "typedef struct bamm_occ bamm_occ;" in hdr and "ScoreSeqSet.cpp:70-126" in hdr


def test_shared_window_formula_gives_the_reference_pvalues(host, g):
    pos, neg = g["occ_pos_mops"], np.sort(g["occ_neg_mops"])
    fp, higher, lower = ranks_and_neighbours(pos, neg)
    assert len(pos) == 11280 and len(neg) == 22560
    p = np.zeros(len(pos), np.float32)
    s_ntop, lam, n_top = C.c_float(), C.c_float(), C.c_uint32()
    lowest = np.ascontiguousarray(neg[:101])
    assert host.bh_occ_window_pvalues(ptr(pos), ptr(fp), ptr(higher), ptr(lower), C.c_uint64(len(pos)), ptr(lowest),
                                      C.c_uint64(len(neg)), ptr(p), C.byref(s_ntop), C.byref(lam), C.byref(n_top)) == 0
    assert n_top.value == 100
    assert np.float32(s_ntop.value) == neg[100]
    want_lambda = np.float32(0)
    for x in neg[:100]:                                       # sequential fp32 sum, ScoreSeqSet.cpp:89-93
        want_lambda = np.float32(want_lambda + np.float32(x - neg[100]))
    assert np.float32(lam.value) == np.float32(want_lambda / np.float32(100))
    assert np.array_equal(p, g["occ_pvalues"])
    # the shape of the fixture the device path's tests rely on
    assert int((p < 0.02).sum()) == 274 and int((fp < 10).sum()) == 20 and fp[p < 0.02].min() >= 10
    # ... and the host path is the same function behind its own sort and search
    p2, e2 = np.zeros(len(pos), np.float32), np.zeros(len(pos), np.float32)
    assert host.bh_mops_pvalues(ptr(pos), C.c_uint64(len(pos)), ptr(np.ascontiguousarray(g["occ_neg_mops"])), C.c_uint64(len(neg)),
                                C.c_uint64(120), ptr(p2), ptr(e2)) == 0
    assert np.array_equal(p2, p) and np.array_equal(e2, p * np.float32(120))


@pytest.mark.parametrize("cutoff", [0.02, 1e-4, 0.5])
def test_hit_list_writer_reproduces_the_occurrence_file(cutoff, host, g, tmp_path):
    pv = g["occ_pvalues"]
    W = int(g["W"])
    codes = np.ascontiguousarray(g["codes"], np.uint8)
    off = np.ascontiguousarray(g["in_off"], np.uint64)
    lw1 = 2 * np.diff(off.astype(np.int64)) + 1 - W + 1       # both strands
    moff = np.concatenate([[0], np.cumsum(lw1)])
    hits = np.flatnonzero(pv < np.float32(cutoff))
    seq = (np.searchsorted(moff, hits, side="right") - 1).astype(np.uint64)
    pos = (hits - moff[seq.astype(np.int64)]).astype(np.uint32)
    p = np.ascontiguousarray(pv[hits])
    e = (p * np.float32(120)).astype(np.float32)
    assert host.bh_occurrence_hits(str(tmp_path).encode(), b"h", ptr(codes), ptr(off), C.c_uint64(120), 0, W, C.c_uint64(len(hits)),
                                   ptr(seq), ptr(pos), ptr(p), ptr(e)) == 0, host.bh_last_error()
    mine = open(tmp_path / "h.occurrence", "rb").read()
    if cutoff == 0.02:
        assert len(hits) == 274 and mine == g["occ_file"].tobytes()
    # the writer that walks a p-value per window is the yardstick at every cut-off
    ev = (pv * np.float32(120)).astype(np.float32)
    assert host.bh_occurrence(str(tmp_path).encode(), b"w", ptr(codes), ptr(off), C.c_uint64(120), 0, W, ptr(np.ascontiguousarray(pv)),
                              ptr(ev), C.c_float(cutoff)) == 0
    assert mine == open(tmp_path / "w.occurrence", "rb").read()
    assert mine.count(b"\n") == 1 + len(hits)
    if cutoff == 1e-4:
        assert len(hits) == 0
    if cutoff == 0.5:
        assert len(hits) == 5530
