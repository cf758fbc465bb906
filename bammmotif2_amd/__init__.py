"""MI355X-native EM refinement hot path of BaMMmotif2.

`csrc/` holds the HIP kernels and the C ABI (include/bamm_em.h); `em.py` mirrors the
reference's EM / ScoreSeqSet interface over that ABI; `synth.py` makes the benchmark inputs.
"""
from . import abi, synth  # noqa: F401
from .em import (EM, Comm, Context, PackedSeqs, SeqSet, calculate_p, logodds, occurrences, Occurrences, FdrMops, fdr_geometry, seed_from_pwm, sample_negatives, libc_srand,  # noqa: F401
                 v_size, v_offset, bg_size, bg_offset, device_count, device_pci_bus_id, device_can_access_peer, peer_access_matrix, device_blocks_live, mask_plan, mix_layout, mix_fix_word, score_tile_geometry, score_slice_geometry, em_tile_geometry, neg_segment_geometry, score_plan,
                 kmer_counts_gapped, kmer_counts_gapped_host, kmer_seeds_gapped)

__all__ = ["EM", "Comm", "Context", "PackedSeqs", "SeqSet", "calculate_p", "logodds", "occurrences", "Occurrences", "FdrMops", "fdr_geometry", "seed_from_pwm", "sample_negatives", "libc_srand",
           "v_size", "v_offset", "bg_size", "bg_offset", "device_count", "device_pci_bus_id", "device_can_access_peer", "peer_access_matrix", "device_blocks_live", "mask_plan", "mix_layout", "mix_fix_word", "score_tile_geometry", "score_slice_geometry", "em_tile_geometry", "neg_segment_geometry", "score_plan",
           "kmer_counts_gapped", "kmer_counts_gapped_host", "kmer_seeds_gapped", "abi", "synth"]
