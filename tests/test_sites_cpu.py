"""EM sites on the device, the parts that need no GPU: the C ABI declares and binds bamm_em_sites and its accessors, and
the .positions writer that takes a site list (host/fdr.cpp, what `--saveBaMMs` feeds from the device) reproduces a numpy
restatement of EM::write's loop (refinement/EM.cpp:585-601) on the responsibilities of the reference's own third pass
(tests/golden: r_2) -- as does the writer that walks dense r (`--hostPositions`)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bammmotif2_amd import abi, build
from tests import golden_util as gu

SITES_SYMBOLS = {"bamm_em_sites": 5, "bamm_sites_info": 3, "bamm_sites_get": 5, "bamm_sites_best": 5, "bamm_sites_destroy": 1,
                 "bamm_em_plan_paths": 4}
CUTOFF = np.float32(0.3)


@pytest.fixture(scope="module")
def host(lib):
    build.build_host()
    H = C.CDLL(build.HOST_LIB)
    H.bh_last_error.restype = C.c_char_p
    return H


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_header_declares_and_abi_binds_the_sites_entry_points(lib):
    hdr = open(os.path.join(os.path.dirname(abi.HERE), "include", "bamm_em.h")).read()
    for name, n_args in SITES_SYMBOLS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/bamm_em.h"
        assert len(m.group(1).split(",")) == n_args, name
        assert name in abi.SYMBOLS
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == n_args, name
    assert "typedef struct bamm_sites bamm_sites;" in hdr and "EM.cpp:577-601" in hdr
    assert "sites.hip" in build.SOURCES and "sites.cpp" in build.SOURCES
    assert '"sites_chunk_positions"' in hdr


def golden_sites(name, key="r_2"):
    """(case, full lengths, r, hit sequences, hit window starts) of a fixture whose golden r covers every sequence."""
    c, g = gu.load(name)
    assert int(g["r_seqs"]) == c.N
    L0 = np.diff(c.in_off.astype(np.int64))
    L = L0 if c.ss else 2 * L0 + 1
    off = np.concatenate([[0], np.cumsum(L)])
    r = np.ascontiguousarray(g[key], np.float32)
    assert len(r) == off[-1]
    seq, pos = [], []
    for n in range(c.N):
        i = np.arange(L[n] - c.W + 1)
        hit = i[r[off[n] + L[n] - c.W - i] >= CUTOFF]           # EM.cpp:590-592
        seq += [n] * len(hit)
        pos += list(hit)
    return c, L, r, np.array(seq, np.uint64), np.array(pos, np.uint32)


def restated_positions_file(c, headers, seq, pos):
    """EM.cpp:581-601 row by row: Sequence::getSequence() is the forward strand, one N, the reverse complement."""
    rows = [b"seq\tlength\tstrand\tstart..end\tpattern\n"]
    base = b"NACGT"
    for n, i in zip(seq.astype(np.int64), pos.astype(np.int64)):
        fwd = c.codes[int(c.in_off[n]):int(c.in_off[n + 1])].astype(np.int64)
        fwd = np.where(fwd <= 4, fwd, 0)
        full = fwd if c.ss else np.concatenate([fwd, [0], np.where(fwd[::-1] > 0, 5 - fwd[::-1], 0)])
        shown = len(fwd)
        pattern = bytes(base[x] for x in full[i:i + c.W])
        rows.append(headers[n] + b"\t%d\t%s\t%d..%d\t" % (shown, b"+" if i < shown else b"-", i + 1, i + c.W) + pattern + b"\n")
    return b"".join(rows)


@pytest.mark.parametrize("name", ["small_k2_ds_N", "small_k0_ss", "small_k3_ds"])
def test_site_list_writer_reproduces_the_positions_file(name, host, tmp_path):
    c, L, r, seq, pos = golden_sites(name)
    assert len(seq) > 0
    has_n = np.array([(c.codes[int(c.in_off[n]):int(c.in_off[n + 1])] == 0).any() for n in range(c.N)])
    if name == "small_k2_ds_N":                                # both strands, a hit on the reverse strand, hits in sequences with N
        assert not c.ss and (pos.astype(np.int64) >= (L[seq.astype(np.int64)] - 1) // 2).any() and has_n[seq.astype(np.int64)].any()
    if name == "small_k0_ss":                                  # single strand, hits in sequences with N
        assert c.ss and has_n[seq.astype(np.int64)].any()
    if name == "small_k3_ds":                                  # several hits on the reverse strand
        assert (pos.astype(np.int64) >= (L[seq.astype(np.int64)] - 1) // 2).sum() >= 2
    headers = [b">%s_%d some text" % (name.encode(), n) for n in range(c.N)]
    want = restated_positions_file(c, headers, seq, pos)
    assert want.count(b"\n") == 1 + len(seq)
    hd = (C.c_char_p * c.N)(*headers)
    codes = np.ascontiguousarray(c.codes, np.uint8)
    off = np.ascontiguousarray(c.in_off, np.uint64)
    assert host.bh_positions_hits(str(tmp_path).encode(), b"hits", hd, ptr(codes), ptr(off), C.c_uint64(c.N), int(c.ss), c.W,
                                  C.c_uint64(len(seq)), ptr(seq), ptr(pos)) == 0, host.bh_last_error()
    assert open(tmp_path / "hits.positions", "rb").read() == want
    # the writer that walks dense r (--hostPositions) gives the same bytes
    assert host.bh_positions(str(tmp_path).encode(), b"dense", hd, ptr(codes), ptr(off), C.c_uint64(c.N), int(c.ss), c.W, ptr(r),
                             C.c_float(0.3)) == 0, host.bh_last_error()
    assert open(tmp_path / "dense.positions", "rb").read() == want


def test_site_list_writer_refuses_a_window_beyond_the_set(host, tmp_path):
    c, L, r, seq, pos = golden_sites("small_k0_ss")
    hd = (C.c_char_p * c.N)(*[b">s"] * c.N)
    codes = np.ascontiguousarray(c.codes, np.uint8)
    off = np.ascontiguousarray(c.in_off, np.uint64)
    for bad_seq, bad_pos in ((c.N, 0), (0, int(L[0]) - c.W + 1)):
        s1, p1 = np.array([bad_seq], np.uint64), np.array([bad_pos], np.uint32)
        assert host.bh_positions_hits(str(tmp_path).encode(), b"bad", hd, ptr(codes), ptr(off), C.c_uint64(c.N), 1, c.W, C.c_uint64(1),
                                      ptr(s1), ptr(p1)) != 0
