"""The launch geometry of bamm_em_mask (csrc/plan.cpp: mask_plan, exported as bamm_mask_plan) against values worked out
by hand from its expressions, one case per branch the planner has.  No GPU: the function is pure.

The expressions, with kLds = 160 KiB = 163840, r16(x) = x rounded up to a multiple of 16, and, for a longest sequence
of L positions,
    wave(L, wide) = 2 * r16(4 L) + r16((wide ? 4 : 2) * L) + r16(4 * (L / 32 + 2))            (mask.hip: mask_wave_bytes)
are
    direct      = r16(8 Y) > kLds
    wave_global = direct or wave(L, narrow) + r16(8 Y) > kLds or L > 65535
    wave_bytes  = wave(L, wave_global)
    s_bytes     = r16(4 W (Y + 1))
    s_in_lds    = s_bytes <= 65536 and (wave_global or s_bytes + wave_bytes <= kLds)
    e_table     = s_in_lds ? s_bytes : 0
    m_cols      = direct ? W : max(1, min(W, (wave_global ? kLds / 2 : min(kLds / 2, kLds - wave_bytes)) / (8 Y)))
    m_table     = direct ? 0 : r16(8 m_cols Y)
    waves(t)    = wave_global ? 4 : max(1, min(4, (kLds - t) / wave_bytes));  e_waves = waves(e_table), m_waves = waves(m_table)
    init_table  = r16(16 W)
    cus         = wave_global ? max(1, min(min(64, CUs), 8 GiB / (32 wave_bytes))) : CUs
    per_cu      = max(1, 16 / min(e_waves, m_waves))
    cap_blocks  = direct ? 8 cus : max(cus, min(cus * per_cu, 64 MiB / (8 cells)))
    mblocks     = max(1, min(ceil(n / min(e_waves, m_waves)), cap_blocks))
    wave_scratch_bytes = wave_global ? max(8 cus, mblocks) * 4 * wave_bytes : 0
"""
import pytest

import bammmotif2_amd as bm

CASES = {
    # K = 2 (Y = 64), W = 20, L = 401, n = 1000, cells = 1280, 256 CUs.
    #   r16(8 * 64) = 512 <= kLds: direct = 0
    #   wave(401, narrow) = 2 * r16(1604) + r16(802) + r16(4 * (12 + 2)) = 2 * 1616 + 816 + 64 = 4112; 4112 + 512 <= kLds and
    #   401 <= 65535: wave_global = 0, wave_bytes = 4112
    #   s_bytes = r16(4 * 20 * 65) = 5200 <= 65536 and 5200 + 4112 <= kLds: s_in_lds = 1, e_table = 5200
    #   m_cols = min(20, min(81920, 163840 - 4112) / 512) = min(20, 160) = 20; m_table = r16(8 * 20 * 64) = 10240
    #   e_waves = min(4, (163840 - 5200) / 4112 = 38) = 4; m_waves = min(4, (163840 - 10240) / 4112 = 37) = 4
    #   init_table = r16(320) = 320; cus = 256; per_cu = 16 / 4 = 4
    #   cap_blocks = max(256, min(1024, 67108864 / 10240 = 6553)) = 1024; mblocks = min(ceil(1000 / 4) = 250, 1024) = 250
    "arrays_in_lds": (dict(W=20, Y=64, max_len=401, n_seqs=1000, cells=1280, num_cus=256),
                      dict(direct=0, wave_global=0, wave_bytes=4112, s_in_lds=1, e_table=5200, m_cols=20, m_table=10240,
                           init_table=320, e_waves=4, m_waves=4, cus=256, mblocks=250, wave_scratch_bytes=0)),
    # The same model, L = 12000: the arrays still fit, but only one wave's worth of them beside a table.
    #   wave(12000, narrow) = 2 * 48000 + 24000 + r16(4 * (375 + 2) = 1508) = 96000 + 24000 + 1520 = 121520;
    #   121520 + 512 <= kLds: wave_global = 0
    #   s_in_lds: 5200 + 121520 = 126720 <= kLds: 1
    #   m_cols = min(20, min(81920, 163840 - 121520 = 42320) / 512 = 82) = 20; m_table = 10240
    #   e_waves = (163840 - 5200) / 121520 = 1; m_waves = (163840 - 10240) / 121520 = 1
    #   per_cu = 16; cap_blocks = max(256, min(4096, 6553)) = 4096; mblocks = min(1000, 4096) = 1000
    "one_wave_per_block": (dict(W=20, Y=64, max_len=12000, n_seqs=1000, cells=1280, num_cus=256),
                           dict(direct=0, wave_global=0, wave_bytes=121520, s_in_lds=1, e_table=5200, m_cols=20, m_table=10240,
                                init_table=320, e_waves=1, m_waves=1, cus=256, mblocks=1000, wave_scratch_bytes=0)),
    # The same model, L = 20000: the arrays go to the global scratch.
    #   wave(20000, narrow) = 2 * 80000 + 40000 + r16(4 * (625 + 2) = 2508) = 160000 + 40000 + 2512 = 202512 > kLds - 512:
    #   wave_global = 1; wave_bytes = wave(20000, wide) = 160000 + 80000 + 2512 = 242512
    #   s_in_lds = 1 (5200 <= 65536, wave_global); e_table = 5200
    #   m_cols = min(20, 81920 / 512 = 160) = 20; m_table = 10240; e_waves = m_waves = 4
    #   cus = min(min(64, 256), 8589934592 / (32 * 242512 = 7760384) = 1106) = 64; per_cu = 4
    #   cap_blocks = max(64, min(256, 6553)) = 256; mblocks = min(250, 256) = 250
    #   wave_scratch_bytes = max(8 * 64 = 512, 250) * 4 * 242512 = 496664576
    "arrays_in_global_scratch": (dict(W=20, Y=64, max_len=20000, n_seqs=1000, cells=1280, num_cus=256),
                                 dict(direct=0, wave_global=1, wave_bytes=242512, s_in_lds=1, e_table=5200, m_cols=20, m_table=10240,
                                      init_table=320, e_waves=4, m_waves=4, cus=64, mblocks=250,
                                      wave_scratch_bytes=512 * 4 * 242512)),
    # K = 7 (Y = 65536), W = 8, L = 401, n = 5000, cells = 524288, 256 CUs.
    #   r16(8 * 65536) = 524288 > kLds: direct = 1, hence wave_global = 1
    #   wave_bytes = wave(401, wide) = 2 * 1616 + r16(1604) + 64 = 3232 + 1616 + 64 = 4912
    #   s_bytes = r16(4 * 8 * 65537 = 2097184) = 2097184 > 65536: s_in_lds = 0, e_table = 0
    #   m_cols = W = 8; m_table = 0; e_waves = m_waves = 4; init_table = r16(128) = 128
    #   cus = min(64, 8589934592 / (32 * 4912 = 157184) = 54649) = 64
    #   cap_blocks = 8 * 64 = 512; mblocks = min(ceil(5000 / 4) = 1250, 512) = 512
    #   wave_scratch_bytes = max(512, 512) * 4 * 4912 = 10059776
    "counts_into_the_accumulator": (dict(W=8, Y=65536, max_len=401, n_seqs=5000, cells=524288, num_cus=256),
                                    dict(direct=1, wave_global=1, wave_bytes=4912, s_in_lds=0, e_table=0, m_cols=8, m_table=0,
                                         init_table=128, e_waves=4, m_waves=4, cus=64, mblocks=512, wave_scratch_bytes=10059776)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_mask_plan_matches_the_hand_derivation(name, lib):
    inputs, want = CASES[name]
    got = bm.mask_plan(**inputs)
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
