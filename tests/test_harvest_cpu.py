"""The resident bins of the mixed-row kernel (csrc/mixed_kernel.h, geometry in csrc/grouped.hip: mix_geometry) have 65 cells
per column: 64 bins and a dump cell that takes the fix lanes' adds of the code "no bin".  No device needed."""
import bammmotif2_amd as bm


def test_no_layout_lost_a_resident_column(lib):
    """65 cells per resident column instead of 64: every width the planner gives mixed rows keeps the columns it had
    (W = 20 at 16 waves is the tight one: 11 columns, 216 bytes of the 160 KiB left)."""
    before = {(13, 7): 13, (14, 7): 14, (16, 7): 16, (17, 7): 17, (20, 7): 11,
              (13, 10): 13, (14, 10): 14, (16, 10): 16, (17, 10): 17, (20, 10): 16}
    for (W, M), n1c in before.items():
        assert bm.mix_layout(W, M)["n1c"] == n1c, (W, M)
