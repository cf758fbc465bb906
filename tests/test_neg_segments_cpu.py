"""The segments bamm_sample_negatives cuts a negative beyond 8192 positions into (bamm_neg_segment_geometry, csrc/negs.hip):
a pure function of nothing, so that tests can place sequence lengths on the cuts.  The segments' generator states come from
rand_jump with the powers t^(2^b) the short records use already -- no power table of its own to check here."""
import ctypes as C

import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import abi


def test_segment_geometry():
    s = bm.neg_segment_geometry()
    assert s > 0 and s % 16 == 0                             # a 2-bit word of 16 bases belongs to one segment
    assert all(bm.neg_segment_geometry() == s for _ in range(3))


def test_segment_geometry_refuses_a_null_output():
    lib = abi.load()
    assert lib.bamm_neg_segment_geometry(None) == abi.ERR_ARG
    with pytest.raises(bm.abi.BammError):
        abi.check(lib.bamm_neg_segment_geometry(None))


def test_header_names_the_function_and_the_tuning_key():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(bm.__file__)), "..", "include", "bamm_em.h")).read()
    assert "bamm_neg_segment_geometry(uint32_t* segment_positions)" in hdr
    assert '"neg_segment_positions"' in hdr
    s = C.c_uint32()
    assert abi.load().bamm_neg_segment_geometry(C.byref(s)) == abi.OK and s.value == bm.neg_segment_geometry()
