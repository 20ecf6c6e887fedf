"""mapad_amd — MI355X-native implementation of the mapAD read-mapping hot path (`mapad map`).

The product is libmapad_amd.so (hand-written HIP kernels for gfx950 behind the C ABI of include/mapad_amd.h).
This package is the thin host-side mirror used by the tests, bench.py and the multi-GPU driver.
"""
import os as _os

# one hardware queue per batch in flight (read by the HIP runtime at its first call; see csrc/mapad_amd.hip: mapad_default_hw_queues)
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

from .binding import (AlleleHost, BatchResult, Context, CoverageHost, DedupHost, Index, MapadError, Params, PileupHost, SnpPanelHost, snp_panel_rule, damage_profile_host, damage_score_host, damage_score_table, quality_rescale_host, quality_rescale_table, hits_to_records, lib, make_params, params_from_cli, allele_quantized_row, genotype_quantized_row, GENOTYPES,
                      alignment_tracks_host, pack_alignments, ALN_CLASSES, Merger, merge_params, merge_pairs_host, trim_reads_host, MERGE_CLASSES, TRIM_CLASSES, Cleaner, clean_params, clean_reads_host, CLEAN_CLASSES, CLEAN_OPS,
                      mappability_host, mappability_summary_host)  # noqa: F401

__all__ = ["AlleleHost", "allele_quantized_row", "genotype_quantized_row", "GENOTYPES", "BatchResult", "Context", "CoverageHost", "DedupHost", "Index", "MapadError", "Params", "PileupHost", "SnpPanelHost", "snp_panel_rule", "damage_profile_host", "damage_score_host", "damage_score_table", "quality_rescale_host", "quality_rescale_table", "hits_to_records", "lib", "make_params", "params_from_cli",
           "alignment_tracks_host", "pack_alignments", "ALN_CLASSES", "Merger", "merge_params", "merge_pairs_host", "trim_reads_host", "MERGE_CLASSES", "TRIM_CLASSES", "Cleaner", "clean_params", "clean_reads_host", "CLEAN_CLASSES", "CLEAN_OPS", "mappability_host", "mappability_summary_host"]
