"""The negative sampler on the device for records beyond 8192 positions (csrc/negs.hip: k_neg_segments; include/bamm_em.h:
bamm_sample_negatives) against the host restatement (host/fdr.cpp::sample_negatives, which the CPU suite pins to the
reference's own negatives).  A long negative is cut into segments of S positions (bamm_neg_segment_geometry), a segment is a
map over the 16 contexts of order 2, the maps are composed: every base must be the host's, so the lengths here sit on the
cuts, and over all the sets the segments' entry contexts -- computed from the host's negatives -- cover all 16 states (a
composition that only worked for some contexts would show)."""
import ctypes as C

import numpy as np
import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import build

pytestmark = pytest.mark.gpu

S = bm.neg_segment_geometry()
K_CUT = 8192 // S + 1                                        # the first k with k S > 8192


@pytest.fixture(scope="module")
def host():
    build.build_host()
    h = C.CDLL(build.HOST_LIB)
    h.bh_last_error.restype = C.c_char_p
    return h


def host_negatives(host, packed, m_fold, generic, stride):
    n, m = C.c_uint64(), C.c_uint64()
    assert host.bh_sample_negatives_strided(packed._p, 2, C.c_uint64(m_fold), int(generic), C.c_uint64(stride), C.byref(n), C.byref(m), None, None) == 0, host.bh_last_error()
    codes, off = np.zeros(m.value, np.uint8), np.zeros(n.value + 1, np.uint64)
    assert host.bh_sample_negatives_strided(packed._p, 2, C.c_uint64(m_fold), int(generic), C.c_uint64(stride), C.byref(n), C.byref(m),
                                            codes.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p)) == 0
    return codes, off


def make_set(lengths, seed, n_at=()):
    """Records of exactly these base counts, uniform bases; n_at: (record, base) pairs set to N (code 0)."""
    rs = np.random.RandomState(seed)
    off = np.zeros(len(lengths) + 1, np.uint64)
    off[1:] = np.cumsum(np.asarray(lengths, np.int64))
    codes = rs.randint(1, 5, size=int(off[-1])).astype(np.uint8)
    for rec, at in n_at:
        codes[int(off[rec]) + at] = 0
    return codes, off


# name, base counts, single strand, N positions, m
CASES = [
    dict(name="ss_8193", lens=[8193, 8193, 8193], ss=True, m=3),
    dict(name="ss_on_the_cut", lens=[K_CUT * S - 1, K_CUT * S, K_CUT * S + 1], ss=True, m=3),
    dict(name="ss_partial_last_word", lens=[2 * S + 17, (K_CUT + 1) * S + 17], ss=True, m=3),
    dict(name="ss_65539", lens=[65539], ss=True, m=3),
    dict(name="ss_257_segments", lens=[257 * S + 5], ss=True, m=1),
    dict(name="ds_4100_N_at_the_junction", lens=[4100, 4100, 4100], ss=False, m=3,
         n_at=[(0, 0), (0, 4099), (0, 2000), (1, 4098), (1, 4099), (2, 1), (2, 777)]),
    dict(name="long_only_m70", lens=[8200, 9000], ss=True, m=70),
    dict(name="mixed_short_before_between_after", lens=[50, 300, 8193, 8192, 17, K_CUT * S + 3, 3 * K_CUT * S, 2, 120, 8191], ss=True, m=3,
         n_at=[(2, 5), (6, 9000)]),
    dict(name="mixed_ds", lens=[100, 4097, 30, 6000, 4096], ss=False, m=1, n_at=[(1, 4096), (3, 0)]),
]
_sets = {}
_seen_contexts = set()


def the_set(case, host, gpu_ctx):
    """The case's positives packed and resident, once for all its parameters."""
    if case["name"] not in _sets:
        codes, off = make_set(case["lens"], 1000 + CASES.index(case), case.get("n_at", ()))
        _sets[case["name"]] = bm.PackedSeqs.from_codes(codes, off, case["ss"], seed=42)
    return _sets[case["name"]]


def note_entry_contexts(want_codes, want_off):
    """The context (two bases) in front of every segment boundary of the host's long negatives."""
    for a, b in zip(want_off[:-1].astype(np.int64), want_off[1:].astype(np.int64)):
        if b - a <= 8192:
            continue
        cut = np.arange(S, b - a, S) + a
        _seen_contexts.update(((want_codes[cut - 2].astype(int) - 1) * 4 + want_codes[cut - 1].astype(int) - 1).tolist())


@pytest.mark.parametrize("generic", [False, True], ids=["seq_specific", "generic"])
@pytest.mark.parametrize("stride", [0, 4, 5])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_long_device_negatives_are_the_host_negatives(case, stride, generic, gpu_ctx, host):
    packed = the_set(case, host, gpu_ctx)
    assert packed.lengths.max() > 8192
    pos = bm.SeqSet(gpu_ctx, packed)
    want_codes, want_off = host_negatives(host, packed, case["m"], generic, stride)
    note_entry_contexts(want_codes, want_off)
    neg, res = bm.sample_negatives(gpu_ctx, pos, 2, case["m"], generic, stride)
    assert neg.n_seqs == len(want_off) - 1
    assert np.array_equal(neg.lengths, np.diff(want_off.astype(np.int64)))
    assert neg.n_exceptions == 0
    got = (neg.unpack_y(0) + 1).astype(np.uint8)             # the 2-bit stream back as codes 1..4
    assert np.array_equal(got, want_codes)
    ref = bm.PackedSeqs.from_codes(want_codes, want_off, True, seed=None)
    assert np.array_equal(ref.words, neg.words)
    res.close(); pos.close()


def test_the_boundaries_met_every_entry_context(gpu_ctx, host):
    """Runs behind the cases above (file order): their segments started in all 16 contexts."""
    if not _seen_contexts:                                   # run on its own: the largest case alone has 257 boundaries
        case = CASES[4]
        note_entry_contexts(*host_negatives(host, the_set(case, host, gpu_ctx), 3, False, 0))
    assert _seen_contexts == set(range(16)), sorted(_seen_contexts)


def test_the_cut_does_not_change_the_negatives(gpu_ctx, host):
    """"neg_segment_positions": the same negatives at other segment lengths (16 = a word per lane; one that is no power of two;
    one longer than the record)."""
    case = CASES[7]
    packed = the_set(case, host, gpu_ctx)
    pos = bm.SeqSet(gpu_ctx, packed)
    want_codes, want_off = host_negatives(host, packed, 2, False, 0)
    try:
        for seg in (16, 48, 1000, 4096, 1 << 20):
            gpu_ctx.set_tuning(neg_segment_positions=seg)
            neg, _ = bm.sample_negatives(gpu_ctx, pos, 2, 2, False, 0, resident=False)
            assert np.array_equal((neg.unpack_y(0) + 1).astype(np.uint8), want_codes), seg
    finally:
        gpu_ctx.set_tuning(neg_segment_positions=0)
    pos.close()
