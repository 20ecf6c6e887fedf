"""ctypes mirror of include/mapad_amd.h (the C ABI of libmapad_amd.so).

Host-side plumbing only: this module never computes alignments itself and has no CPU fallback — every mapping call goes
through the HIP library and raises MapadError if the library or a gfx950 device is missing.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

_HERE = os.path.dirname(os.path.abspath(__file__))


class MapadError(RuntimeError):
    CODES = {-1: "invalid argument", -2: "I/O error", -3: "index version mismatch", -4: "parse error", -5: "no gfx950 device (no CPU fallback)",
             -6: "HIP call failed", -7: "out of memory", -8: "read too long", -9: "input beyond a documented limit of this entry point"}

    def __init__(self, code, what=""):
        self.code = code
        super().__init__(f"{what}: {self.CODES.get(code, 'error')} ({code})")


class Params(C.Structure):
    """mapad_params_t"""
    _fields_ = [
        ("model_kind", C.c_int32), ("library_prep", C.c_int32),
        ("five_prime_overhang", C.c_float), ("three_prime_overhang", C.c_float),
        ("ds_deamination_rate", C.c_float), ("ss_deamination_rate", C.c_float), ("divergence", C.c_float),
        ("ignore_base_quality", C.c_int32),
        ("deam_score", C.c_float), ("mm_score", C.c_float), ("match_score", C.c_float),
        ("bound_kind", C.c_int32),
        ("poisson_threshold", C.c_float), ("base_error_rate", C.c_float),
        ("cutoff", C.c_float), ("exponent", C.c_float),
        ("threshold", C.c_float), ("repr_mm_bound", C.c_float),
        ("penalty_gap_open", C.c_float), ("penalty_gap_extend", C.c_float),
        ("gap_dist_ends", C.c_int32), ("max_num_gaps_open", C.c_int32), ("stack_limit_abort", C.c_int32),
        ("stack_limit", C.c_uint32), ("edit_tree_limit", C.c_uint32),
        ("chunk_size", C.c_uint64),
    ]


class Hit(C.Structure):
    """mapad_hit_t"""
    _fields_ = [("lower", C.c_uint64), ("lower_rev", C.c_uint64), ("size", C.c_uint64), ("alignment_score", C.c_float),
                ("n_ops", C.c_uint32), ("ops_offset", C.c_uint32), ("reserved", C.c_uint32)]


HIT_DTYPE = np.dtype([("lower", "<u8"), ("lower_rev", "<u8"), ("size", "<u8"), ("score", "<f4"), ("n_ops", "<u4"), ("ops_offset", "<u4"), ("reserved", "<u4")])
COUNTER_DTYPE = np.dtype([("e_search", "<u4"), ("e_darray", "<u4"), ("n_push", "<u4"), ("n_pop", "<u4"), ("n_node", "<u4"), ("n_hits", "<u4")])
assert HIT_DTYPE.itemsize == C.sizeof(Hit) == 40


class BatchResultC(C.Structure):
    """mapad_batch_result_t"""
    _fields_ = [("n_reads", C.c_uint64), ("n_hits", C.c_uint64), ("n_ops", C.c_uint64), ("hit_begin", C.c_void_p), ("hits", C.c_void_p),
                ("ops", C.c_void_p), ("status", C.c_void_p), ("counters", C.c_void_p), ("d_arrays", C.c_void_p), ("n_second_pass", C.c_uint64), ("n_third_pass", C.c_uint64)]


class RecordC(C.Structure):
    """mapad_record_t"""
    _fields_ = [("flags", C.c_uint16), ("mapq", C.c_uint8), ("mapped", C.c_uint8), ("reverse", C.c_uint8), ("tid", C.c_int32), ("pos", C.c_int64),
                ("as_score", C.c_float), ("xs_score", C.c_float), ("nm", C.c_int32), ("x0", C.c_int32), ("x1", C.c_int32), ("has_xs", C.c_uint8),
                ("xt", C.c_char), ("cigar_off", C.c_uint32), ("cigar_len", C.c_uint32), ("md_off", C.c_uint32), ("md_len", C.c_uint32),
                ("xa_off", C.c_uint32), ("xa_len", C.c_uint32)]


class RecordsC(C.Structure):
    _fields_ = [("n", C.c_uint64), ("recs", C.POINTER(RecordC)), ("text", C.c_void_p), ("text_len", C.c_uint64)]


DAMAGE_POSITIONS = 32


class DamageProfileC(C.Structure):
    """mapad_damage_profile_t"""
    _fields_ = [("counts", C.c_uint64 * (2 * DAMAGE_POSITIONS * 16)), ("reads", C.c_uint64), ("reads_seen", C.c_uint64), ("aligned_bases", C.c_uint64),
                ("skipped_bases", C.c_uint64), ("insertions", C.c_uint64), ("deletions", C.c_uint64), ("batches", C.c_uint64), ("kernel_ms", C.c_double)]


COVERAGE_BINS = 256


class CoverageContigC(C.Structure):
    """mapad_coverage_contig_t"""
    _fields_ = [("length", C.c_uint64), ("reads", C.c_uint64), ("covered_bases", C.c_uint64), ("depth_sum", C.c_uint64), ("max_depth", C.c_uint64)]


class CoverageC(C.Structure):
    """mapad_coverage_t"""
    _fields_ = [("n_contigs", C.c_uint32), ("pad", C.c_uint32), ("contigs", C.POINTER(CoverageContigC)), ("hist", C.c_uint64 * COVERAGE_BINS), ("reads", C.c_uint64),
                ("reads_seen", C.c_uint64), ("covered_columns", C.c_uint64), ("deleted_columns", C.c_uint64), ("insertions", C.c_uint64), ("batches", C.c_uint64),
                ("accumulate_ms", C.c_double), ("summary_ms", C.c_double)]


MAPPABILITY_BINS = 9
MAPPABILITY_VERIFY = 1


class MappabilityContigC(C.Structure):
    """mapad_mappability_contig_t"""
    _fields_ = [("length", C.c_uint64), ("valid_starts", C.c_uint64), ("unique_starts", C.c_uint64), ("hist", C.c_uint64 * MAPPABILITY_BINS), ("majority", C.c_uint64),
                ("strict", C.c_uint64)]


class MappabilityC(C.Structure):
    """mapad_mappability_t"""
    _fields_ = [("n_contigs", C.c_uint32), ("k", C.c_uint32), ("e", C.c_uint32), ("pad", C.c_uint32), ("contigs", C.POINTER(MappabilityContigC)),
                ("total", MappabilityContigC), ("starts", C.c_uint64), ("steps", C.c_uint64), ("kernel_ms", C.c_double)]


class PileupContigC(C.Structure):
    """mapad_pileup_contig_t"""
    _fields_ = [("length", C.c_uint64), ("sites_covered", C.c_uint64), ("sites_deep", C.c_uint64), ("sites_called", C.c_uint64), ("called", C.c_uint64 * 4),
                ("base_sum", C.c_uint64 * 4), ("max_depth", C.c_uint64)]


class PileupC(C.Structure):
    """mapad_pileup_t"""
    _fields_ = [("n_contigs", C.c_uint32), ("pad", C.c_uint32), ("contigs", C.POINTER(PileupContigC)), ("mode", C.c_uint32), ("min_base_quality", C.c_uint32),
                ("mask5", C.c_uint32), ("mask3", C.c_uint32), ("min_depth", C.c_uint32), ("min_percent", C.c_uint32), ("reads", C.c_uint64), ("reads_seen", C.c_uint64),
                ("columns_counted", C.c_uint64), ("columns_not_acgt", C.c_uint64), ("columns_masked", C.c_uint64), ("columns_low_quality", C.c_uint64),
                ("deleted_columns", C.c_uint64), ("insertions", C.c_uint64), ("batches", C.c_uint64), ("accumulate_ms", C.c_double), ("summary_ms", C.c_double)]


class SnpPanelRuleC(C.Structure):
    """mapad_snp_panel_rule_t"""
    _fields_ = [("call", C.c_uint32), ("min_depth", C.c_uint32), ("transitions", C.c_uint32), ("seed", C.c_uint64)]


SNP_PANEL_SCALARS = ("reads_seen", "reads", "reads_on_panel", "columns_counted", "columns_not_acgt", "columns_masked", "columns_low_quality", "columns_deleted")
SNP_PANEL_WORDS = ("rows", "rows_unplaced", "rows_bad_alleles", "rows_transition", "rows_covered", "rows_called", "called_ref", "called_alt", "transitions_called",
                   "obs_ref", "obs_alt", "obs_other", "max_depth")
SNP_PANEL_CALLS = {"random": 0, "majority": 1}
SNP_PANEL_TRANSITIONS = {"keep": 0, "missing": 1, "single_strand": 2}


class SnpPanelC(C.Structure):
    """mapad_snp_panel_t"""
    _fields_ = ([("mode", C.c_uint32), ("min_base_quality", C.c_uint32), ("mask5", C.c_uint32), ("mask3", C.c_uint32), ("rule", SnpPanelRuleC), ("n_rows", C.c_uint64),
                 ("n_slots", C.c_uint64)] + [(k, C.c_uint64) for k in SNP_PANEL_SCALARS + SNP_PANEL_WORDS]
                + [("batches", C.c_uint64), ("accumulate_ms", C.c_double), ("summary_ms", C.c_double)])


class AlleleContigC(C.Structure):
    """mapad_allele_contig_t"""
    _fields_ = [("length", C.c_uint64), ("sites_covered", C.c_uint64), ("sites_deep", C.c_uint64), ("sites_called", C.c_uint64), ("called", C.c_uint64 * 4),
                ("max_depth", C.c_uint64), ("margin_sum_q", C.c_uint64)]


class AlleleC(C.Structure):
    """mapad_allele_t"""
    _fields_ = [("n_contigs", C.c_uint32), ("pad", C.c_uint32), ("contigs", C.POINTER(AlleleContigC)), ("mode", C.c_uint32), ("min_base_quality", C.c_uint32),
                ("mask5", C.c_uint32), ("mask3", C.c_uint32), ("min_depth", C.c_uint32), ("min_margin_q", C.c_int32), ("reads", C.c_uint64), ("reads_seen", C.c_uint64),
                ("columns_counted", C.c_uint64), ("columns_not_acgt", C.c_uint64), ("columns_masked", C.c_uint64), ("columns_low_quality", C.c_uint64),
                ("deleted_columns", C.c_uint64), ("insertions", C.c_uint64), ("batches", C.c_uint64), ("accumulate_ms", C.c_double), ("summary_ms", C.c_double)]


class GenotypeContigC(C.Structure):
    """mapad_genotype_contig_t"""
    _fields_ = [("length", C.c_uint64), ("sites_covered", C.c_uint64), ("sites_deep", C.c_uint64), ("sites_called", C.c_uint64), ("called", C.c_uint64 * 10),
                ("max_depth", C.c_uint64), ("margin_sum_q", C.c_uint64)]


class GenotypeC(C.Structure):
    """mapad_genotype_t"""
    _fields_ = [("n_contigs", C.c_uint32), ("on", C.c_uint32), ("contigs", C.POINTER(GenotypeContigC)), ("min_depth", C.c_uint32), ("min_margin_q", C.c_int32),
                ("het_penalty_q", C.c_int32), ("pad", C.c_uint32), ("batches", C.c_uint64), ("accumulate_ms", C.c_double), ("summary_ms", C.c_double)]


GENOTYPES = ("AA", "CC", "GG", "TT", "AC", "AG", "AT", "CG", "CT", "GT")
GENOTYPE_NO_CALL = 255
DUPLICATES_BINS = 256


class DuplicatesC(C.Structure):
    """mapad_duplicates_t"""
    _fields_ = [("reads_seen", C.c_uint64), ("reads_eligible", C.c_uint64), ("duplicates", C.c_uint64), ("fragments", C.c_uint64), ("slots", C.c_uint64),
                ("grows", C.c_uint64), ("batches", C.c_uint64), ("histogram", C.c_uint64 * DUPLICATES_BINS), ("mark_ms", C.c_double), ("summary_ms", C.c_double)]


DAMAGE_SCORE_BINS = 128


class DamageScoresC(C.Structure):
    """mapad_damage_scores_t"""
    _fields_ = [("reads_seen", C.c_uint64), ("reads_scored", C.c_uint64), ("reads_below", C.c_uint64), ("informative_columns", C.c_uint64), ("score_sum", C.c_int64),
                ("batches", C.c_uint64), ("threshold_q", C.c_int32), ("pad", C.c_int32), ("histogram", C.c_uint64 * DAMAGE_SCORE_BINS), ("kernel_ms", C.c_double)]


RESCALE_BINS = 64


class RescaleC(C.Structure):
    """mapad_rescale_t"""
    _fields_ = [("reads_seen", C.c_uint64), ("reads_rescaled", C.c_uint64), ("candidate_columns", C.c_uint64 * 2), ("bases_changed", C.c_uint64),
                ("quality_drop_sum", C.c_uint64), ("new_quality", C.c_uint64 * RESCALE_BINS), ("batches", C.c_uint64), ("kernel_ms", C.c_double)]


ALN_CLASSES = ("ok", "unmapped", "below_min_mapq", "no_md", "bad_contig", "unsupported_cigar", "length_mismatch", "md_mismatch", "off_contig")
# mapad_alignment_t
ALIGNMENT_DTYPE = np.dtype([("pos0", "<i8"), ("x0", "<u8"), ("cigar_off", "<u8"), ("md_off", "<u8"), ("tid", "<i4"), ("n_cigar", "<u4"), ("md_len", "<u4"), ("as_score", "<f4"),
                            ("flags", "<u2"), ("mapq", "u1"), ("pad0", "u1"), ("pad1", "<u4")])
assert ALIGNMENT_DTYPE.itemsize == 56


class AlnResultC(C.Structure):
    """mapad_aln_result_t"""
    _fields_ = [("n_reads", C.c_uint64), ("status_class", C.c_void_p), ("duplicate", C.c_void_p), ("scored", C.c_void_p), ("score_q", C.c_void_p),
                ("rescaled_quals", C.c_void_p), ("n_quals", C.c_uint64), ("class_counts", C.c_uint64 * len(ALN_CLASSES)), ("build_ms", C.c_float)]


class TracksC(C.Structure):
    """mapad_tracks_t"""
    _fields_ = [("n_reads", C.c_uint64), ("n_ops", C.c_uint64), ("hit_begin", C.c_void_p), ("hits", C.c_void_p), ("ops", C.c_void_p), ("status_class", C.c_void_p),
                ("mapped", C.c_void_p), ("error", C.c_void_p), ("best", C.c_void_p), ("x0", C.c_void_p), ("tid", C.c_void_p), ("rel", C.c_void_p), ("abs", C.c_void_p),
                ("backward", C.c_void_p), ("class_counts", C.c_uint64 * len(ALN_CLASSES))]


MERGE_CLASSES = ("merged", "too_short", "unmerged", "empty_mate", "too_long")
TRIM_CLASSES = ("trimmed", "too_short", "untouched", "empty_mate", "too_long")  # the same five in single-end mode
MERGE_HIST_BINS = 1025
MERGE_MAX_MATE_LEN = 512
MERGE_MAX_ADAPTER = 64


class MergeParamsC(C.Structure):
    """mapad_merge_params_t"""
    _fields_ = [("min_overlap", C.c_uint32), ("min_adapter_overlap", C.c_uint32), ("max_mismatch_permille", C.c_uint32), ("min_length", C.c_uint32),
                ("max_quality", C.c_uint32), ("adapter1_len", C.c_uint32), ("adapter2_len", C.c_uint32), ("mode", C.c_uint32),
                ("adapter1", C.c_uint8 * MERGE_MAX_ADAPTER), ("adapter2", C.c_uint8 * MERGE_MAX_ADAPTER)]


class MergeCountsC(C.Structure):
    """mapad_merge_counts_t"""
    _fields_ = [("pairs_seen", C.c_uint64), ("class_counts", C.c_uint64 * len(MERGE_CLASSES)), ("bases_in", C.c_uint64), ("bases_out", C.c_uint64),
                ("histogram", C.c_uint64 * MERGE_HIST_BINS), ("calls", C.c_uint64)]


class MergeResultC(C.Structure):
    """mapad_merge_result_t"""
    _fields_ = [("n_pairs", C.c_uint64), ("total_bases", C.c_uint64), ("cls", C.c_void_p), ("frag_len", C.c_void_p), ("matches", C.c_void_p), ("mismatches", C.c_void_p),
                ("seqs", C.c_void_p), ("quals", C.c_void_p), ("offsets", C.c_void_p), ("counts", MergeCountsC), ("kernel_ms", C.c_float * 2)]


CLEAN_CLASSES = ("kept", "trimmed", "too_short", "low_complexity", "empty", "too_long")
CLEAN_OPS = {"poly": 1, "trim_n": 2, "trim_qual": 4, "dust": 8}
CLEAN_MAX_LEN = 1024
CLEAN_LEN_BINS = 1025
CLEAN_DUST_BINS = 101


class CleanParamsC(C.Structure):
    """mapad_clean_params_t"""
    _fields_ = [("ops", C.c_uint32), ("poly_base", C.c_uint32), ("poly_min_len", C.c_uint32), ("poly_one_in", C.c_uint32), ("poly_max_mismatch", C.c_uint32),
                ("min_quality", C.c_uint32), ("min_length", C.c_uint32), ("max_dust", C.c_uint32)]


class CleanCountsC(C.Structure):
    """mapad_clean_counts_t"""
    _fields_ = [("reads_seen", C.c_uint64), ("class_counts", C.c_uint64 * len(CLEAN_CLASSES)), ("bases_in", C.c_uint64), ("bases_out", C.c_uint64),
                ("bases_poly", C.c_uint64), ("bases_trim5", C.c_uint64), ("bases_trim3", C.c_uint64), ("length_histogram", C.c_uint64 * CLEAN_LEN_BINS),
                ("dust_histogram", C.c_uint64 * CLEAN_DUST_BINS), ("calls", C.c_uint64)]


class CleanResultC(C.Structure):
    """mapad_clean_result_t"""
    _fields_ = [("n_reads", C.c_uint64), ("total_bases", C.c_uint64), ("cls", C.c_void_p), ("trim5", C.c_void_p), ("trim3", C.c_void_p), ("poly_len", C.c_void_p),
                ("dust", C.c_void_p), ("seqs", C.c_void_p), ("quals", C.c_void_p), ("offsets", C.c_void_p), ("counts", CleanCountsC), ("kernel_ms", C.c_float * 2)]


MODEL_KINDS = {"simple_adna": 0, "vindija_pwm": 1, "test": 2}
BOUND_KINDS = {"discrete": 0, "continuous": 1, "test": 2}
LIBRARY_PREPS = {"single_stranded": 0, "double_stranded": 1}

# every symbol include/mapad_amd.h declares: name -> (restype, argtypes)
_vp, _u64, _u32, _i32, _f, _u8 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_float, C.c_uint8
_PP = C.POINTER(Params)
SYMBOLS = {
    "mapad_version": (C.c_char_p, []),
    "mapad_params_from_cli": (_i32, [_PP, _i32, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _i32, _i32, _i32, _i32, _u64]),
    "mapad_sdm_get": (_f, [_PP, _u64, _u64, _u8, _u8, _u8]),
    "mapad_sdm_representative_mismatch_penalty": (_f, [_PP]),
    "mapad_sdm_min_penalty": (_f, [_PP, _u64, _u64, _u8, _u8, _i32]),
    "mapad_sdm_alignment_start": (_i32, [_PP, _u64]),
    "mapad_mb_reject": (_i32, [_PP, _f, _u64]),
    "mapad_mb_reject_iterative": (_i32, [_PP, _f, _f]),
    "mapad_mb_remaining_frac_of_repr_mm": (_f, [_PP, _f, _u64]),
    "mapad_index_build": (_i32, [_vp, _vp, _vp, _u32, _u64, C.POINTER(_vp)]),
    "mapad_index_build_gpu": (_i32, [_vp, _vp, _vp, _u32, _u64, _i32, C.POINTER(_vp)]),
    "mapad_last_index_build_info": (_i32, [_vp]),
    "mapad_index_open": (_i32, [C.c_char_p, C.POINTER(_vp)]),
    "mapad_index_save": (_i32, [_vp, C.c_char_p]),
    "mapad_index_free": (None, [_vp]),
    "mapad_index_text_len": (_u64, [_vp]),
    "mapad_index_copy_bwt": (_i32, [_vp, _vp]),
    "mapad_index_n_contigs": (_u32, [_vp]),
    "mapad_index_contig": (_i32, [_vp, _u32, C.POINTER(C.c_char_p), C.POINTER(_u64), C.POINTER(_u64)]),
    "mapad_index_sa_sample_len": (_u64, [_vp]),
    "mapad_index_sa_extra_len": (_u64, [_vp]),
    "mapad_index_copy_sa": (_i32, [_vp, _vp, _vp, _vp]),
    "mapad_index_device_view": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_u64), _vp, _vp]),
    "mapad_index_sa_get": (_i32, [_vp, _u64, C.POINTER(_u64)]),
    "mapad_index_sa_get_batch": (_i32, [_vp, _vp, _u64, _vp]),
    "mapad_ctx_create": (_i32, [_vp, _PP, _i32, C.POINTER(_vp)]),
    "mapad_ctx_destroy": (None, [_vp]),
    "mapad_ctx_set_stream": (_i32, [_vp, _vp]),
    "mapad_ctx_set_fetch_d_arrays": (_i32, [_vp, _i32]),
    "mapad_ctx_set_collapse_duplicates": (_i32, [_vp, _i32]),
    "mapad_last_collapse_info": (_i32, [_vp, _vp]),
    "mapad_ctx_prepare_lengths": (_i32, [_vp, _vp, _u32]),
    "mapad_map_batch": (_i32, [_vp, _vp, _vp, _vp, _u64, C.POINTER(C.POINTER(BatchResultC))]),
    "mapad_batch_result_free": (None, [C.POINTER(BatchResultC)]),
    "mapad_submit_batch": (_i32, [_vp, _vp, _vp, _vp, _u64]),
    "mapad_host_alloc": (_vp, [C.c_size_t]),
    "mapad_host_free": (None, [_vp]),
    "mapad_map_batch_device": (_i32, [_vp, _vp, _vp, _vp, _u64, _u32]),
    "mapad_fetch_result": (_i32, [_vp, C.POINTER(C.POINTER(BatchResultC))]),
    "mapad_ctx_set_pipeline_depth": (_i32, [_vp, _i32]),
    "mapad_ctx_select_batch": (_i32, [_vp, _i32]),
    "mapad_ctx_reserve": (_i32, [_vp, _u64, _u64, _u32, _i32]),
    "mapad_kernel_history": (_i32, [_vp, _vp, _u32, C.POINTER(_u32)]),
    "mapad_compact_result_device": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_u64), C.POINTER(_u64)]),
    "mapad_device_result_ptrs": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "mapad_last_batch_counters": (_i32, [_vp, _vp]),
    "mapad_last_kernel_ms": (_i32, [_vp, _vp]),
    "mapad_last_launch_info": (_i32, [_vp, _vp]),
    "mapad_host_cpus": (C.c_uint32, []),
    "mapad_ctx_set_reserved_cus": (_i32, [_vp, C.c_int32]),
    "mapad_ctx_set_tail_pops": (_i32, [_vp, C.c_uint32]),
    "mapad_tail_set_local_world": (C.c_uint32, [C.c_uint32]),
    "mapad_last_tail_info": (_i32, [_vp, _vp]),
    "mapad_hits_to_records": (_i32, [_vp, _PP, C.POINTER(BatchResultC), _vp, _vp, _vp, _vp, _u64, C.POINTER(C.POINTER(RecordsC))]),
    "mapad_records_free": (None, [C.POINTER(RecordsC)]),
    "mapad_records_seed_at": (_u64, [_u64, _u64]),
    "mapad_sa_locate": (_i32, [_vp, _vp, _u64, _vp]),
    "mapad_last_locate_info": (_i32, [_vp, C.POINTER(C.c_float), C.POINTER(_u64), C.POINTER(_u64)]),
    "mapad_hits_to_records_gpu": (_i32, [_vp, C.POINTER(BatchResultC), _vp, _vp, _vp, _vp, _u64, C.POINTER(C.POINTER(RecordsC))]),
    "mapad_records_device": (_i32, [_vp, _u64, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_u64), C.POINTER(_u64)]),
    "mapad_hits_to_coords_gpu": (_i32, [_vp, C.POINTER(BatchResultC), _u64, C.POINTER(_vp)]),
    "mapad_coords_to_records": (_i32, [_vp, _PP, C.POINTER(BatchResultC), _vp, _vp, C.POINTER(C.POINTER(RecordsC))]),
    "mapad_coords_free": (None, [_vp]),
    "mapad_ctx_set_damage_profile": (_i32, [_vp, _i32]),
    "mapad_ctx_damage_profile": (_i32, [_vp, C.POINTER(DamageProfileC)]),
    "mapad_ctx_damage_profile_reset": (_i32, [_vp]),
    "mapad_damage_profile_host": (_i32, [_vp, _PP, C.POINTER(BatchResultC), _vp, _vp, _u64, _i32, C.POINTER(DamageProfileC)]),
    "mapad_ctx_set_coverage": (_i32, [_vp, _i32]),
    "mapad_ctx_coverage": (_i32, [_vp, C.POINTER(CoverageC)]),
    "mapad_ctx_coverage_depth": (_i32, [_vp, C.c_uint32, _u64, _u64, _vp]),
    "mapad_ctx_coverage_reset": (_i32, [_vp]),
    "mapad_ctx_coverage_merge": (_i32, [_vp, _vp]),
    "mapad_coverage_host_new": (_i32, [_vp, _i32, C.POINTER(_vp)]),
    "mapad_coverage_host_add": (_i32, [_vp, _vp, _PP, C.POINTER(BatchResultC), _u64]),
    "mapad_coverage_host_summary": (_i32, [_vp, C.POINTER(CoverageC)]),
    "mapad_coverage_host_depth": (_i32, [_vp, C.c_uint32, _u64, _u64, _vp]),
    "mapad_coverage_host_free": (None, [_vp]),
    "mapad_ctx_set_pileup": (_i32, [_vp, _i32, _u32, _u32, _u32]),
    "mapad_ctx_pileup": (_i32, [_vp, _u32, _u32, C.POINTER(PileupC)]),
    "mapad_ctx_pileup_counts": (_i32, [_vp, _u32, _u64, _u64, _vp]),
    "mapad_ctx_pileup_consensus": (_i32, [_vp, _u32, _u64, _u64, _u32, _u32, _vp]),
    "mapad_ctx_pileup_reset": (_i32, [_vp]),
    "mapad_ctx_pileup_merge": (_i32, [_vp, _vp]),
    "mapad_pileup_host_new": (_i32, [_vp, _i32, _u32, _u32, _u32, C.POINTER(_vp)]),
    "mapad_pileup_host_add": (_i32, [_vp, _vp, _PP, C.POINTER(BatchResultC), _vp, _vp, _vp, _u64]),
    "mapad_pileup_host_summary": (_i32, [_vp, _u32, _u32, C.POINTER(PileupC)]),
    "mapad_pileup_host_counts": (_i32, [_vp, _u32, _u64, _u64, _vp]),
    "mapad_pileup_host_consensus": (_i32, [_vp, _u32, _u64, _u64, _u32, _u32, _vp]),
    "mapad_pileup_host_free": (None, [_vp]),
    "mapad_ctx_set_mark_duplicates": (_i32, [_vp, _i32]),
    "mapad_ctx_duplicates": (_i32, [_vp, C.POINTER(DuplicatesC)]),
    "mapad_ctx_duplicates_reset": (_i32, [_vp]),
    "mapad_dedup_host_new": (_i32, [C.POINTER(_vp)]),
    "mapad_dedup_host_add": (_i32, [_vp, _vp, _PP, C.POINTER(BatchResultC), _u64, _vp]),
    "mapad_dedup_host_summary": (_i32, [_vp, C.POINTER(DuplicatesC)]),
    "mapad_dedup_host_free": (None, [_vp]),
    "mapad_damage_profile_host_skip": (_i32, [_vp, _PP, C.POINTER(BatchResultC), _vp, _vp, _u64, _i32, _vp, C.POINTER(DamageProfileC)]),
    "mapad_coverage_host_add_skip": (_i32, [_vp, _vp, _PP, C.POINTER(BatchResultC), _u64, _vp]),
    "mapad_pileup_host_add_skip": (_i32, [_vp, _vp, _PP, C.POINTER(BatchResultC), _vp, _vp, _vp, _u64, _vp]),
    "mapad_ctx_set_damage_score": (_i32, [_vp, _i32, _f]),
    "mapad_ctx_damage_scores": (_i32, [_vp, C.POINTER(DamageScoresC)]),
    "mapad_ctx_damage_scores_reset": (_i32, [_vp]),
    "mapad_records_damage_scores": (_i32, [C.POINTER(RecordsC), C.POINTER(_vp), C.POINTER(_vp)]),
    "mapad_damage_score_host": (_i32, [_vp, _PP, C.POINTER(BatchResultC), _vp, _vp, _vp, _u64, _f, _vp, _vp, C.POINTER(DamageScoresC)]),
    "mapad_damage_score_table": (_i32, [_PP, _u32, _vp, C.POINTER(C.c_int)]),
    "mapad_ctx_set_quality_rescale": (_i32, [_vp, _i32]),
    "mapad_ctx_quality_rescale": (_i32, [_vp, C.POINTER(RescaleC)]),
    "mapad_ctx_quality_rescale_reset": (_i32, [_vp]),
    "mapad_records_rescaled_quals": (_i32, [C.POINTER(RecordsC), C.POINTER(_vp), C.POINTER(_u64)]),
    "mapad_quality_rescale_host": (_i32, [_vp, _PP, C.POINTER(BatchResultC), _vp, _vp, _vp, _u64, _vp, C.POINTER(RescaleC)]),
    "mapad_quality_rescale_table": (_i32, [_PP, _u32, _vp]),
    "mapad_ctx_set_allele_likelihoods": (_i32, [_vp, _i32, _u32, _u32, _u32]),
    "mapad_ctx_allele_summary": (_i32, [_vp, _u32, _f, C.POINTER(AlleleC)]),
    "mapad_ctx_allele_cells": (_i32, [_vp, _u32, _u64, _u64, _vp, _vp]),
    "mapad_ctx_allele_consensus": (_i32, [_vp, _u32, _u64, _u64, _u32, _f, _vp, _vp]),
    "mapad_ctx_allele_reset": (_i32, [_vp]),
    "mapad_ctx_allele_merge": (_i32, [_vp, _vp]),
    "mapad_allele_host_new": (_i32, [_vp, _i32, _u32, _u32, _u32, C.POINTER(_vp)]),
    "mapad_allele_host_add": (_i32, [_vp, _vp, _PP, C.POINTER(BatchResultC), _vp, _vp, _vp, _u64]),
    "mapad_allele_host_add_skip": (_i32, [_vp, _vp, _PP, C.POINTER(BatchResultC), _vp, _vp, _vp, _u64, _vp]),
    "mapad_allele_host_summary": (_i32, [_vp, _u32, _f, C.POINTER(AlleleC)]),
    "mapad_allele_host_cells": (_i32, [_vp, _u32, _u64, _u64, _vp, _vp]),
    "mapad_allele_host_consensus": (_i32, [_vp, _u32, _u64, _u64, _u32, _f, _vp, _vp]),
    "mapad_allele_host_free": (None, [_vp]),
    "mapad_allele_quantized_row": (_i32, [_PP, _u32, _u32, _u32, _u32, _vp]),
    "mapad_ctx_set_genotype_likelihoods": (_i32, [_vp, _i32]),
    "mapad_ctx_genotype_summary": (_i32, [_vp, _u32, _f, _f, C.POINTER(GenotypeC)]),
    "mapad_ctx_genotype_cells": (_i32, [_vp, _u32, _u64, _u64, _vp]),
    "mapad_ctx_genotype_calls": (_i32, [_vp, _u32, _u64, _u64, _u32, _f, _f, _vp, _vp]),
    "mapad_ctx_genotype_merge": (_i32, [_vp, _vp]),
    "mapad_genotype_quantized_row": (_i32, [_PP, _u32, _u32, _u32, _u32, _vp]),
    "mapad_allele_host_set_genotypes": (_i32, [_vp, _i32]),
    "mapad_allele_host_genotype_summary": (_i32, [_vp, _u32, _f, _f, C.POINTER(GenotypeC)]),
    "mapad_allele_host_genotype_cells": (_i32, [_vp, _u32, _u64, _u64, _vp]),
    "mapad_allele_host_genotype_calls": (_i32, [_vp, _u32, _u64, _u64, _u32, _f, _f, _vp, _vp]),
    "mapad_ctx_set_snp_panel": (_i32, [_vp, _i32, _u64, _vp, _vp, _vp, _vp, _u32, _u32, _u32]),
    "mapad_ctx_snp_panel": (_i32, [_vp, C.POINTER(SnpPanelRuleC), C.POINTER(SnpPanelC)]),
    "mapad_ctx_snp_panel_counts": (_i32, [_vp, _u64, _u64, _vp]),
    "mapad_ctx_snp_panel_calls": (_i32, [_vp, _u64, _u64, C.POINTER(SnpPanelRuleC), _vp]),
    "mapad_ctx_snp_panel_reset": (_i32, [_vp]),
    "mapad_ctx_snp_panel_merge": (_i32, [_vp, _vp]),
    "mapad_snp_panel_host_new": (_i32, [_vp, _i32, _u64, _vp, _vp, _vp, _vp, _u32, _u32, _u32, C.POINTER(_vp)]),
    "mapad_snp_panel_host_add": (_i32, [_vp, _vp, _PP, C.POINTER(BatchResultC), _vp, _vp, _vp, _u64]),
    "mapad_snp_panel_host_add_skip": (_i32, [_vp, _vp, _PP, C.POINTER(BatchResultC), _vp, _vp, _vp, _u64, _vp]),
    "mapad_snp_panel_host_summary": (_i32, [_vp, C.POINTER(SnpPanelRuleC), C.POINTER(SnpPanelC)]),
    "mapad_snp_panel_host_counts": (_i32, [_vp, _u64, _u64, _vp]),
    "mapad_snp_panel_host_calls": (_i32, [_vp, _u64, _u64, C.POINTER(SnpPanelRuleC), _vp]),
    "mapad_snp_panel_host_free": (None, [_vp]),
    "mapad_ctx_accumulate_alignments": (_i32, [_vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _u32, C.POINTER(C.POINTER(AlnResultC))]),
    "mapad_aln_result_free": (None, [C.POINTER(AlnResultC)]),
    "mapad_ctx_alignment_tracks": (_i32, [_vp, C.POINTER(C.POINTER(TracksC))]),
    "mapad_alignment_tracks_host": (_i32, [_vp, _PP, _vp, _u64, _vp, _vp, _vp, _u32, C.POINTER(C.POINTER(TracksC))]),
    "mapad_tracks_free": (None, [C.POINTER(TracksC)]),
    "mapad_merge_params_default": (None, [C.POINTER(MergeParamsC)]),
    "mapad_merge_params_check": (_i32, [C.POINTER(MergeParamsC)]),
    "mapad_merger_create": (_i32, [_i32, C.POINTER(MergeParamsC), C.POINTER(_vp)]),
    "mapad_merger_set_stream": (_i32, [_vp, _vp]),
    "mapad_merger_free": (None, [_vp]),
    "mapad_merge_pairs": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(C.POINTER(MergeResultC))]),
    "mapad_trim_reads": (_i32, [_vp, _vp, _vp, _vp, _u64, C.POINTER(C.POINTER(MergeResultC))]),
    "mapad_merge_result_free": (None, [C.POINTER(MergeResultC)]),
    "mapad_merger_totals": (_i32, [_vp, C.POINTER(MergeCountsC)]),
    "mapad_merger_reset": (_i32, [_vp]),
    "mapad_merge_counts_add": (None, [C.POINTER(MergeCountsC), C.POINTER(MergeCountsC)]),
    "mapad_merge_pairs_device": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_u64)]),
    "mapad_merge_pairs_host": (_i32, [C.POINTER(MergeParamsC), _vp, _vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(C.POINTER(MergeResultC))]),
    "mapad_trim_reads_host": (_i32, [C.POINTER(MergeParamsC), _vp, _vp, _vp, _u64, C.POINTER(C.POINTER(MergeResultC))]),
    "mapad_clean_params_default": (None, [C.POINTER(CleanParamsC)]),
    "mapad_clean_params_check": (_i32, [C.POINTER(CleanParamsC)]),
    "mapad_cleaner_create": (_i32, [_i32, C.POINTER(CleanParamsC), C.POINTER(_vp)]),
    "mapad_cleaner_set_stream": (_i32, [_vp, _vp]),
    "mapad_cleaner_free": (None, [_vp]),
    "mapad_clean_reads": (_i32, [_vp, _vp, _vp, _vp, _u64, C.POINTER(C.POINTER(CleanResultC))]),
    "mapad_clean_result_free": (None, [C.POINTER(CleanResultC)]),
    "mapad_cleaner_totals": (_i32, [_vp, C.POINTER(CleanCountsC)]),
    "mapad_cleaner_reset": (_i32, [_vp]),
    "mapad_clean_counts_add": (None, [C.POINTER(CleanCountsC), C.POINTER(CleanCountsC)]),
    "mapad_clean_reads_device": (_i32, [_vp, _vp, _vp, _vp, _u64, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_u64)]),
    "mapad_clean_reads_host": (_i32, [C.POINTER(CleanParamsC), _vp, _vp, _vp, _u64, C.POINTER(C.POINTER(CleanResultC))]),
    "mapad_ctx_mappability": (_i32, [_vp, C.c_uint32, _vp, _u64, _u64, _u64, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp]),
    "mapad_ctx_mappability_summary": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_u64), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(MappabilityC)]),
    "mapad_last_mappability_info": (_i32, [_vp, C.POINTER(C.c_double), C.POINTER(_u64), C.POINTER(_u64)]),
    "mapad_mappability_host": (_i32, [_vp, C.c_uint32, _vp, _u64, _u64, _u64, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp]),
    "mapad_mappability_summary_host": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_u64), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(MappabilityC)]),
}

_lib = None


def lib():
    """Loads libmapad_amd.so (building it in-tree if the sources are newer).  Raises if it cannot be loaded."""
    global _lib
    if _lib is None:
        path = os.environ.get("MAPAD_AMD_LIB")  # an alternative build of the library (profiling / A-B variants)
        if not path:
            hv = _build.selected_variant()  # MAPAD_HEAP_VARIANT=1..3: the library built with another reading of the heap's tie rules (csrc/heap_core.hpp)
            path = _build.lib_path(hv)
            if _build.needs_build(hv):
                path = _build.build(heap_variant=hv)
        L = C.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            try:
                fn = getattr(L, name)  # AttributeError = the library does not export what the header declares
            except AttributeError:
                if os.environ.get("MAPAD_AMD_LIB") and os.environ.get("MAPAD_AMD_LIB_OLD_ABI"):  # an A/B run against an older build of the library (profiles/dev/ab3.sh)
                    continue
                raise
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        raise MapadError(rc, what)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def make_params(d):
    p = Params()
    d = dict(d)
    p.model_kind = MODEL_KINDS[d.pop("model")]
    p.bound_kind = BOUND_KINDS[d.pop("bound")]
    p.library_prep = LIBRARY_PREPS[d.pop("library", "single_stranded")]
    for k, v in d.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def params_from_cli(library="single_stranded", five_prime_overhang=0.0, three_prime_overhang=0.0, ds_deamination_rate=0.0, ss_deamination_rate=0.0,
                    divergence=0.02, poisson_prob=0.03, as_cutoff=0.0, as_cutoff_exponent=1.0, indel_rate=0.001, gap_extension_penalty=1.0,
                    gap_dist_ends=5, max_num_gaps_open=2, ignore_base_quality=False, no_search_limit_recovery=False, chunk_size=250000):
    """build_alignment_parameters (src/main.rs:418-499); poisson_prob=None selects the Continuous bound."""
    p = Params()
    _check(lib().mapad_params_from_cli(C.byref(p), LIBRARY_PREPS[library], five_prime_overhang, three_prime_overhang, ds_deamination_rate,
                                       ss_deamination_rate, divergence, -1.0 if poisson_prob is None else poisson_prob, as_cutoff, as_cutoff_exponent,
                                       indel_rate, gap_extension_penalty, gap_dist_ends, max_num_gaps_open, int(ignore_base_quality),
                                       int(no_search_limit_recovery), chunk_size), "mapad_params_from_cli")
    return p


class BatchResult:
    """Owns a mapad_batch_result_t and exposes it as numpy views (copied, so the C object can be freed)."""

    def __init__(self, cptr, free_fn):
        r = cptr.contents
        self.n_reads, self.n_hits, self.n_ops = int(r.n_reads), int(r.n_hits), int(r.n_ops)
        self.n_second_pass, self.n_third_pass = int(r.n_second_pass), int(r.n_third_pass)

        def arr(ptr, dtype, n):
            if n == 0 or not ptr:
                return np.zeros(0, dtype=dtype)
            return np.frombuffer((C.c_char * (np.dtype(dtype).itemsize * n)).from_address(ptr), dtype=dtype).copy()

        self.hit_begin = arr(r.hit_begin, np.uint64, self.n_reads + 1)
        self.hits_arr = arr(r.hits, HIT_DTYPE, self.n_hits)
        self.ops = arr(r.ops, np.uint32, self.n_ops)
        self.status = arr(r.status, np.uint32, self.n_reads)
        self.counters = arr(r.counters, COUNTER_DTYPE, self.n_reads)
        total = 0
        self._cptr, self._free = cptr, free_fn
        self._d_ptr = r.d_arrays
        self._arr = arr

    def d_arrays(self, offsets):
        total = int(offsets[-1])
        return self._arr(self._d_ptr, np.float32, total)

    def hits(self, read):
        """hits of one read in BinaryHeap array order: list of {"interval", "score", "ops_raw"}"""
        out = []
        for h in self.hits_arr[int(self.hit_begin[read]):int(self.hit_begin[read + 1])]:
            ops = self.ops[int(h["ops_offset"]):int(h["ops_offset"]) + int(h["n_ops"])]
            out.append({"interval": (int(h["lower"]), int(h["lower_rev"]), int(h["size"])), "score": np.float32(h["score"]), "ops_raw": ops.copy()})
        return out

    def close(self):
        if self._cptr is not None:
            self._free(self._cptr)
            self._cptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Index:
    def __init__(self, handle):
        self.h = handle

    @classmethod
    def build(cls, contigs, seed=1234, device=None):
        """contigs: list of (name: str, seq: bytes / uint8 array).  device=None: suffix sorting on the host (SA-IS);
        device=k: on GPU k (mapad_index_build_gpu) — same index, byte for byte."""
        n = len(contigs)
        names = (C.c_char_p * n)(*[c[0].encode() for c in contigs])
        bufs = [np.ascontiguousarray(np.frombuffer(c[1], dtype=np.uint8) if isinstance(c[1], (bytes, bytearray)) else c[1], dtype=np.uint8) for c in contigs]
        seqs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        lens = (C.c_uint64 * n)(*[b.size for b in bufs])
        out = C.c_void_p()
        if device is None:
            _check(lib().mapad_index_build(names, seqs, lens, n, seed, C.byref(out)), "mapad_index_build")
        else:
            _check(lib().mapad_index_build_gpu(names, seqs, lens, n, seed, int(device), C.byref(out)), "mapad_index_build_gpu")
        return cls(out)

    @staticmethod
    def last_build_info():
        """What the prefix doubling of the most recent build(device=k) of this process did (mapad_last_index_build_info): rounds, unresolved rows before round 1, chunks sorted,
        chunks by the way their end was found (cut at the last head / at the first head behind the limit / uncut tail / whole list), largest chunk, collection pieces, limits."""
        out = np.zeros(16, np.uint64)
        _check(lib().mapad_last_index_build_info(_ptr(out)), "mapad_last_index_build_info")
        return dict(zip(("rounds", "unresolved", "chunks", "cut_last_head", "cut_first_head", "tails", "whole", "largest_chunk", "pieces", "chunk_limit", "sort_cap"), (int(x) for x in out)))

    @classmethod
    def open(cls, prefix):
        out = C.c_void_p()
        _check(lib().mapad_index_open(prefix.encode(), C.byref(out)), "mapad_index_open")
        return cls(out)

    def save(self, prefix):
        _check(lib().mapad_index_save(self.h, prefix.encode()), "mapad_index_save")

    def __del__(self):
        try:
            if self.h:
                lib().mapad_index_free(self.h)
                self.h = None
        except Exception:
            pass

    def __len__(self):
        return int(lib().mapad_index_text_len(self.h))

    def bwt(self):
        out = np.empty(len(self), dtype=np.uint8)
        _check(lib().mapad_index_copy_bwt(self.h, _ptr(out)), "mapad_index_copy_bwt")
        return out

    def contigs(self):
        out = []
        for i in range(lib().mapad_index_n_contigs(self.h)):
            name, s, e = C.c_char_p(), C.c_uint64(), C.c_uint64()
            _check(lib().mapad_index_contig(self.h, i, C.byref(name), C.byref(s), C.byref(e)), "mapad_index_contig")
            out.append((name.value.decode(), s.value, e.value))
        return out

    def sampled_sa(self):
        ns, ne = int(lib().mapad_index_sa_sample_len(self.h)), int(lib().mapad_index_sa_extra_len(self.h))
        sample, er, ev = np.zeros(ns, np.uint64), np.zeros(max(ne, 1), np.uint64), np.zeros(max(ne, 1), np.uint64)
        _check(lib().mapad_index_copy_sa(self.h, _ptr(sample), _ptr(er), _ptr(ev)), "mapad_index_copy_sa")
        return sample, er[:ne], ev[:ne]

    def sa_get(self, row):
        out = C.c_uint64()
        _check(lib().mapad_index_sa_get(self.h, row, C.byref(out)), "mapad_index_sa_get")
        return out.value

    def sa_get_batch(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        out = np.zeros(rows.size, np.uint64)
        _check(lib().mapad_index_sa_get_batch(self.h, _ptr(rows) if rows.size else None, rows.size, _ptr(out) if rows.size else None), "mapad_index_sa_get_batch")
        return out

    def device_view(self):
        blocks, nb = C.c_void_p(), C.c_uint64()
        less, sent = np.zeros(8, np.uint64), np.zeros(2, np.uint64)
        _check(lib().mapad_index_device_view(self.h, C.byref(blocks), C.byref(nb), _ptr(less), _ptr(sent)), "mapad_index_device_view")
        return blocks.value, nb.value, less, sent

    def blocks(self):
        """the rank blocks (8 x u64 per 96 rows) as a numpy view of the index's host copy"""
        ptr, nb, _, _ = self.device_view()
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint64)), shape=(int(nb) * 8,))


class Context:
    """One GPU with the index resident in HBM (mapad_ctx_t)."""

    def __init__(self, index, params, device_id=0):
        self.index, self.params = index, params
        out = C.c_void_p()
        _check(lib().mapad_ctx_create(index.h, C.byref(params), device_id, C.byref(out)), "mapad_ctx_create")
        self.h = out

    def close(self):
        if self.h:
            lib().mapad_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        _check(lib().mapad_ctx_set_stream(self.h, stream_ptr), "mapad_ctx_set_stream")

    def set_fetch_d_arrays(self, on):
        _check(lib().mapad_ctx_set_fetch_d_arrays(self.h, int(on)), "mapad_ctx_set_fetch_d_arrays")

    def set_collapse_duplicates(self, on):
        """Map each distinct read of a batch once (same length, bases and — unless ignored — qualities); results are unchanged.  Default off."""
        _check(lib().mapad_ctx_set_collapse_duplicates(self.h, int(on)), "mapad_ctx_set_collapse_duplicates")

    def collapse_info(self):
        """(reads, groups = reads searched, reads that had a twin, key collisions kept apart by the byte compare, pops executed, grouping us, fan-out us, 0) of the
        selected batch; pops and the fan-out time once it has been collected.  Collapsing off: (n, n, 0, 0, 0, 0, 0, 0)."""
        out = np.zeros(8, np.uint64)
        _check(lib().mapad_last_collapse_info(self.h, _ptr(out)), "mapad_last_collapse_info")
        return [int(x) for x in out]

    def set_damage_profile(self, mode):
        """Damage profile of the batches converted to records from now on: 0 off (default), 1 all mapped reads, 2 reads with X0 == 1 only.  Starts an empty table."""
        _check(lib().mapad_ctx_set_damage_profile(self.h, int(mode)), "mapad_ctx_set_damage_profile")

    def damage_profile(self):
        """The table so far: {"counts": uint64[2 (from 5', from 3'), 32 (distance), 4 (reference ACGT), 4 (read ACGT)], "reads", "reads_seen", "aligned_bases",
        "skipped_bases", "insertions", "deletions", "batches", "kernel_ms"}; waits for the batches in flight."""
        out = DamageProfileC()
        _check(lib().mapad_ctx_damage_profile(self.h, C.byref(out)), "mapad_ctx_damage_profile")
        return _damage_dict(out)

    def reset_damage_profile(self):
        _check(lib().mapad_ctx_damage_profile_reset(self.h), "mapad_ctx_damage_profile_reset")

    def set_coverage(self, mode):
        """Depth of coverage of the batches converted to records from now on: 0 off (default), 1 all mapped reads, 2 reads with X0 == 1 only.  Starts an empty table;
        the first switch-on allocates 4 bytes per forward-strand text position on the device."""
        _check(lib().mapad_ctx_set_coverage(self.h, int(mode)), "mapad_ctx_set_coverage")

    def coverage(self):
        """The summary so far: {"contigs": [{"name", "length", "reads", "covered_bases", "depth_sum", "max_depth"}, ...] in index order, "hist": uint64[256] (contig
        positions by depth, the last bin >= 255), "reads", "reads_seen", "covered_columns", "deleted_columns", "insertions", "batches", "accumulate_ms", "summary_ms"};
        waits for the batches in flight."""
        return _coverage_summary(self.index, lambda out: _check(lib().mapad_ctx_coverage(self.h, out), "mapad_ctx_coverage"))

    def coverage_depth(self, tid, start, n):
        """per-base depth of [start, start + n) of contig tid (0-based) as uint32[n]"""
        out = np.zeros(int(n), np.uint32)
        _check(lib().mapad_ctx_coverage_depth(self.h, int(tid), int(start), int(n), _ptr(out) if n else None), "mapad_ctx_coverage_depth")
        return out

    def reset_coverage(self):
        _check(lib().mapad_ctx_coverage_reset(self.h), "mapad_ctx_coverage_reset")

    def merge_coverage(self, other):
        """adds `other`'s accumulator (same index, same mode) into this context's; `other` keeps its own"""
        _check(lib().mapad_ctx_coverage_merge(self.h, other.h), "mapad_ctx_coverage_merge")

    def set_pileup(self, mode, min_bq=0, mask5=0, mask3=0):
        """Pileup (A/C/G/T counts per forward-strand reference position) of the batches converted to records from now on: 0 off (default; frees the array), 1 all
        mapped reads, 2 reads with X0 == 1 only.  min_bq: raw Phred below which a base is left out; mask5 / mask3: bases at the read's 5' / 3' end left out.
        Starts an empty table; the switch-on allocates 16 bytes per forward-strand text position on the device."""
        _check(lib().mapad_ctx_set_pileup(self.h, int(mode), int(min_bq), int(mask5), int(mask3)), "mapad_ctx_set_pileup")

    def pileup(self, min_depth=1, min_percent=0):
        """The summary so far under the call rule (min_depth, min_percent): {"contigs": [{"name", "length", "sites_covered", "sites_deep", "sites_called",
        "called": [A, C, G, T], "base_sum": [A, C, G, T], "max_depth"}, ...] in index order, "mode", "min_base_quality", "mask5", "mask3", "min_depth",
        "min_percent", "reads", "reads_seen", "columns_counted", "columns_not_acgt", "columns_masked", "columns_low_quality", "deleted_columns", "insertions",
        "batches", "accumulate_ms", "summary_ms"}; waits for the batches in flight."""
        return _pileup_summary(self.index, lambda out: _check(lib().mapad_ctx_pileup(self.h, int(min_depth), int(min_percent), out), "mapad_ctx_pileup"))

    def pileup_counts(self, tid, start, n):
        """the counts of [start, start + n) of contig tid (0-based) as uint32[n, 4]: A, C, G, T (forward-strand bases)"""
        out = np.zeros((int(n), 4), np.uint32)
        _check(lib().mapad_ctx_pileup_counts(self.h, int(tid), int(start), int(n), _ptr(out) if n else None), "mapad_ctx_pileup_counts")
        return out

    def pileup_consensus(self, tid, start, n, min_depth=1, min_percent=0):
        """the calls of [start, start + n) of contig tid as uint8[n]: ord of 'A', 'C', 'G', 'T' or 'N'"""
        out = np.zeros(int(n), np.uint8)
        _check(lib().mapad_ctx_pileup_consensus(self.h, int(tid), int(start), int(n), int(min_depth), int(min_percent), _ptr(out) if n else None),
               "mapad_ctx_pileup_consensus")
        return out

    def pileup_reset(self):
        _check(lib().mapad_ctx_pileup_reset(self.h), "mapad_ctx_pileup_reset")

    def pileup_merge(self, other):
        """adds `other`'s counts (same index, mode and filters) into this context's; `other` keeps its own"""
        _check(lib().mapad_ctx_pileup_merge(self.h, other.h), "mapad_ctx_pileup_merge")

    def set_snp_panel(self, mode, tid=None, pos0=None, ref=None, alt=None, min_bq=0, mask5=0, mask3=0):
        """SNP panel (strand-split A/C/G/T counts at the rows' positions, one pseudo-haploid call per row) of the batches converted to records from now on: 0 off
        (default; frees the panel), 1 all mapped reads, 2 X0 == 1 only.  tid / pos0 (0-based on the contig) / ref / alt (ASCII, bytes or uint8): one entry per
        row.  min_bq / mask5 / mask3: the pileup's filters, all 0 by default.  Starts an empty table."""
        if not int(mode):
            _check(lib().mapad_ctx_set_snp_panel(self.h, 0, 0, None, None, None, None, 0, 0, 0), "mapad_ctx_set_snp_panel")
            return
        keep = _panel_rows(tid, pos0, ref, alt)
        _check(lib().mapad_ctx_set_snp_panel(self.h, int(mode), keep[0].size, *(_ptr(a) for a in keep), int(min_bq), int(mask5), int(mask3)), "mapad_ctx_set_snp_panel")

    def snp_panel(self, rule=None):
        """The panel's summary under a call rule (snp_panel_rule(); default: random draw, min_depth 1, transitions kept, seed 0): the settings, the read and
        column counters, the row statistics of panel_core.hpp, batches, accumulate_ms (HIP-event time of panel_kernel over the batches), summary_ms."""
        return _panel_summary(lambda r, out: _check(lib().mapad_ctx_snp_panel(self.h, r, out), "mapad_ctx_snp_panel"), rule)

    def snp_panel_counts(self, row_from, n):
        """uint32[n, 2, 4]: strand (0 forward, 1 reverse), then A, C, G, T, of rows [row_from, row_from + n); zeroes for an unplaced row"""
        out = np.zeros((int(n), 2, 4), np.uint32)
        _check(lib().mapad_ctx_snp_panel_counts(self.h, int(row_from), int(n), _ptr(out) if n else None), "mapad_ctx_snp_panel_counts")
        return out

    def snp_panel_calls(self, row_from, n, rule=None):
        """uint8[n]: ord of '2' (ref), '0' (alt) or '9' (missing) for rows [row_from, row_from + n), in row order"""
        out = np.zeros(int(n), np.uint8)
        r = snp_panel_rule(**(rule or {}))
        _check(lib().mapad_ctx_snp_panel_calls(self.h, int(row_from), int(n), C.byref(r), _ptr(out) if n else None), "mapad_ctx_snp_panel_calls")
        return out

    def snp_panel_reset(self):
        _check(lib().mapad_ctx_snp_panel_reset(self.h), "mapad_ctx_snp_panel_reset")

    def snp_panel_merge(self, other):
        """adds the other context's panel counts into this one's (same index, mode, filters and panel); the other keeps its own"""
        _check(lib().mapad_ctx_snp_panel_merge(self.h, other.h), "mapad_ctx_snp_panel_merge")

    def set_allele_likelihoods(self, mode, min_bq=0, mask5=0, mask3=0):
        """Allele likelihoods (damage-aware haploid consensus) of the batches converted to records from now on: 0 off (default; frees the arrays), 1 all mapped
        reads, 2 reads with X0 == 1 only.  Every counted column adds the damage model's log2 P(read base | allele, position in the read, base quality) for each of
        the four alleles, in units of 1/256 bit.  min_bq / mask5 / mask3: the pileup's filters, all 0 by default.  Starts an empty table; the switch-on allocates
        20 bytes per forward-strand text position on the device."""
        _check(lib().mapad_ctx_set_allele_likelihoods(self.h, int(mode), int(min_bq), int(mask5), int(mask3)), "mapad_ctx_set_allele_likelihoods")

    def allele_summary(self, min_depth=1, min_margin=3.0):
        """The summary so far under the call rule (min_depth, min_margin bits): {"contigs": [{"name", "length", "sites_covered", "sites_deep", "sites_called",
        "called": [A, C, G, T], "max_depth", "margin_sum_q"}, ...] in index order, "mode", "min_base_quality", "mask5", "mask3", "min_depth", "min_margin_q", "reads",
        "reads_seen", "columns_counted", "columns_not_acgt", "columns_masked", "columns_low_quality", "deleted_columns", "insertions", "batches", "accumulate_ms",
        "summary_ms"}; waits for the batches in flight."""
        return _allele_summary(self.index, lambda out: _check(lib().mapad_ctx_allele_summary(self.h, int(min_depth), float(min_margin), out), "mapad_ctx_allele_summary"))

    def allele_cells(self, tid, start, n):
        """(int32[n, 4] log-likelihoods by allele A, C, G, T in 1/256 bit, uint32[n] depth) of [start, start + n) of contig tid (0-based)"""
        ll, depth = np.zeros((int(n), 4), np.int32), np.zeros(int(n), np.uint32)
        _check(lib().mapad_ctx_allele_cells(self.h, int(tid), int(start), int(n), _ptr(ll) if n else None, _ptr(depth) if n else None), "mapad_ctx_allele_cells")
        return ll, depth

    def allele_consensus(self, tid, start, n, min_depth=1, min_margin=3.0):
        """(uint8[n] calls: ord of 'A', 'C', 'G', 'T' or 'N'; uint8[n] qualities: whole bits of margin, 0 for N) of [start, start + n) of contig tid"""
        bases, quals = np.zeros(int(n), np.uint8), np.zeros(int(n), np.uint8)
        _check(lib().mapad_ctx_allele_consensus(self.h, int(tid), int(start), int(n), int(min_depth), float(min_margin), _ptr(bases) if n else None,
                                                _ptr(quals) if n else None), "mapad_ctx_allele_consensus")
        return bases, quals

    def allele_reset(self):
        _check(lib().mapad_ctx_allele_reset(self.h), "mapad_ctx_allele_reset")

    def allele_merge(self, other):
        """adds `other`'s cells and depths (same index, mode and filters) into this context's; `other` keeps its own"""
        _check(lib().mapad_ctx_allele_merge(self.h, other.h), "mapad_ctx_allele_merge")

    def set_genotype_likelihoods(self, on):
        """Diploid genotype likelihoods on top of the allele likelihoods (set_allele_likelihoods with a non-zero mode first: MapadError otherwise): every
        counted column also adds its value under the six heterozygous pairs AC AG AT CG CT GT into int32 het[pos][6]; the four homozygous values are the allele
        cells.  Switching it on or off starts both tables empty; on allocates 24 bytes per forward-strand text position on the device."""
        _check(lib().mapad_ctx_set_genotype_likelihoods(self.h, 1 if on else 0), "mapad_ctx_set_genotype_likelihoods")

    def genotype_summary(self, min_depth=1, min_margin=3.0, het_penalty=0.0):
        """The genotype calls so far under the rule (min_depth, min_margin bits, het_penalty bits): {"contigs": [{"name", "length", "sites_covered", "sites_deep",
        "sites_called", "called": [AA CC GG TT AC AG AT CG CT GT], "max_depth", "margin_sum_q"}, ...], "on", "min_depth", "min_margin_q", "het_penalty_q", "batches",
        "accumulate_ms", "summary_ms"}; waits for the batches in flight."""
        return _genotype_summary(self.index, lambda out: _check(lib().mapad_ctx_genotype_summary(self.h, int(min_depth), float(min_margin), float(het_penalty), out),
                                                                "mapad_ctx_genotype_summary"))

    def genotype_cells(self, tid, start, n):
        """int32[n, 6]: the heterozygous cells AC AG AT CG CT GT (1/256 bit) of [start, start + n) of contig tid; allele_cells() has the homozygous four and the depth"""
        het = np.zeros((int(n), 6), np.int32)
        _check(lib().mapad_ctx_genotype_cells(self.h, int(tid), int(start), int(n), _ptr(het) if n else None), "mapad_ctx_genotype_cells")
        return het

    def genotype_calls(self, tid, start, n, min_depth=1, min_margin=3.0, het_penalty=0.0):
        """(uint8[n] genotypes: index into GENOTYPES, 255 = no call; uint8[n] GQ 0..99) of [start, start + n) of contig tid"""
        gt, gq = np.zeros(int(n), np.uint8), np.zeros(int(n), np.uint8)
        _check(lib().mapad_ctx_genotype_calls(self.h, int(tid), int(start), int(n), int(min_depth), float(min_margin), float(het_penalty), _ptr(gt) if n else None,
                                              _ptr(gq) if n else None), "mapad_ctx_genotype_calls")
        return gt, gq

    def genotype_merge(self, other):
        """adds `other`'s het cells (feature on in both, same index and allele settings) into this context's — after allele_merge, which adds the rest"""
        _check(lib().mapad_ctx_genotype_merge(self.h, other.h), "mapad_ctx_genotype_merge")

    def set_mark_duplicates(self, mode):
        """PCR duplicates by alignment coordinates (start, reference span, strand) among the batches converted to records from now on: 0 off (default; frees the
        table), 1 marks them (0x400 in the record's flags, "duplicate" in its dict), 2 marks them and leaves them out of the damage profile, the coverage and the
        pileup.  The first read in conversion order is the original.  Starts an empty table."""
        _check(lib().mapad_ctx_set_mark_duplicates(self.h, int(mode)), "mapad_ctx_set_mark_duplicates")

    def duplicates(self):
        """{"reads_seen", "reads_eligible", "duplicates", "fragments", "slots", "grows", "batches", "histogram": uint64[256] (bin k: fragments seen k times, the last
        bin >= 255), "mark_ms", "summary_ms"}; waits for the batches in flight."""
        out = DuplicatesC()
        _check(lib().mapad_ctx_duplicates(self.h, C.byref(out)), "mapad_ctx_duplicates")
        return _duplicates_dict(out)

    def duplicates_reset(self):
        _check(lib().mapad_ctx_duplicates_reset(self.h), "mapad_ctx_duplicates_reset")

    def set_damage_score(self, mode, threshold=0.0):
        """Damage score of the reads of the batches converted to records from now on: the log-likelihood ratio, in bits, of a read's reported alignment under the
        damage model (-f / -t / -d / -s) against the same model without damage.  0 off (default), 1 scores ("damage_score" in the record dicts), 2 scores and leaves
        the reads whose score is below `threshold` out of the damage profile, the coverage and the pileup.  Starts an empty summary."""
        _check(lib().mapad_ctx_set_damage_score(self.h, int(mode), float(threshold)), "mapad_ctx_set_damage_score")

    def damage_scores(self):
        """{"reads_seen", "reads_scored", "reads_below", "informative_columns", "score_sum" (of score_q, 1/256 bit), "batches", "threshold_q", "histogram": uint64[128]
        (half a bit per bin, bin 64 starts at 0), "kernel_ms"}; waits for the batches in flight."""
        out = DamageScoresC()
        _check(lib().mapad_ctx_damage_scores(self.h, C.byref(out)), "mapad_ctx_damage_scores")
        return _damage_scores_dict(out)

    def reset_damage_scores(self):
        _check(lib().mapad_ctx_damage_scores_reset(self.h), "mapad_ctx_damage_scores_reset")

    def set_quality_rescale(self, mode):
        """Quality rescaling of the batches converted to records from now on: the base qualities of C->T / G->A mismatches of the reported alignments marked down
        by the posterior, under the damage model (-f / -t / -d / -s), that the mismatch is damage (mapDamage's rule).  0 off (default), 1 rescales the qualities that
        travel with the records (hits_to_records(..., rescaled=True)), 2 also lets the pileup's min_base_quality filter see them.  Starts an empty summary."""
        _check(lib().mapad_ctx_set_quality_rescale(self.h, int(mode)), "mapad_ctx_set_quality_rescale")

    def quality_rescale(self):
        """{"reads_seen", "reads_rescaled", "candidate_columns": uint64[2] (C->T, G->A), "bases_changed", "quality_drop_sum", "new_quality": uint64[64] (changed
        bases by min(q', 63)), "batches", "kernel_ms"}; waits for the batches in flight."""
        out = RescaleC()
        _check(lib().mapad_ctx_quality_rescale(self.h, C.byref(out)), "mapad_ctx_quality_rescale")
        return _rescale_dict(out)

    def reset_quality_rescale(self):
        _check(lib().mapad_ctx_quality_rescale_reset(self.h), "mapad_ctx_quality_rescale_reset")

    def mappability(self, tid, seq, start=0, n=None, k=35, e=0, verify=False, counts=True, cover=True):
        """Loci of the reference's k-mers on the GPU: for the starts / positions [start, start + n) of contig `tid` (n None: to its end) the pair (counts, cover) of
        uint8 arrays — counts[i]: places of the reference, both strands, where the k-mer starting at start + i occurs with at most e substitutions, saturated at 255,
        0 where there is no k-mer of A, C, G, T; cover[i]: the unique k-mers (count 1) that lie over position start + i.  `seq`: the whole contig (bytes or uint8
        array) as the index was built from it.  verify: every search runs to its end, MapadError(-1) if seq is not the index's sequence.  An array not asked for is None."""
        return _mappability(lambda *a: lib().mapad_ctx_mappability(self.h, *a), "mapad_ctx_mappability", tid, seq, start, n, k, e, verify, counts, cover)

    def mappability_summary(self, seqs, k=35, e=0, verify=False):
        """Per-contig and total figures of the mappability of the whole reference (`seqs`: every contig, index order), reduced on the GPU: a dict with k, e, contigs
        (name, length, valid_starts, unique_starts, hist — valid starts by count: 1, 2, 3-4, 5-8, 9-16, 17-32, 33-64, 65-128, >= 129 —, majority, strict), total,
        starts, steps (extension steps, two rank queries each) and kernel_ms."""
        return _mappability_summary(self.index, seqs, k, e, verify, lambda *a: lib().mapad_ctx_mappability_summary(self.h, *a), "mapad_ctx_mappability_summary")

    def mappability_info(self):
        """(kernel_ms, starts, steps) of the latest mappability call on this context"""
        ms, starts, steps = C.c_double(), C.c_uint64(), C.c_uint64()
        _check(lib().mapad_last_mappability_info(self.h, C.byref(ms), C.byref(starts), C.byref(steps)), "mapad_last_mappability_info")
        return float(ms.value), int(starts.value), int(steps.value)

    def prepare_lengths(self, lens):
        a = np.ascontiguousarray(lens, dtype=np.uint32)
        _check(lib().mapad_ctx_prepare_lengths(self.h, _ptr(a), a.size), "mapad_ctx_prepare_lengths")

    def accumulate_alignments(self, seqs, quals, offsets, alns, cigar_words, md_bytes, min_mapq=0):
        """mapad_ctx_accumulate_alignments: the switched-on stages over existing alignments (pack_alignments makes the three arrays), no search.  Reads and
        qualities as map_batch takes them.  -> {"status_class" uint8[n], "class_counts" {name: count}, "build_ms", "duplicate" uint8[n] | None, "scored" uint8[n] |
        None, "score_q" int32[n] | None, "rescaled" uint8[bases] | None}"""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        alns, cigar_words, md_bytes = _alignment_arrays(alns, cigar_words, md_bytes, offsets.size - 1)
        out = C.POINTER(AlnResultC)()
        _check(lib().mapad_ctx_accumulate_alignments(self.h, _ptr(seqs), _ptr(quals), _ptr(offsets), offsets.size - 1, _ptr(alns), _ptr(cigar_words), _ptr(md_bytes),
                                                     int(min_mapq), C.byref(out)), "mapad_ctx_accumulate_alignments")
        try:
            r = out.contents
            n = int(r.n_reads)

            def arr(p, count, dtype):
                return None if not p else np.frombuffer(C.string_at(p, count * np.dtype(dtype).itemsize), dtype).copy()

            return {"status_class": arr(r.status_class, n, np.uint8) if n else np.zeros(0, np.uint8),
                    "class_counts": {k: int(r.class_counts[i]) for i, k in enumerate(ALN_CLASSES)}, "build_ms": float(r.build_ms),
                    "duplicate": arr(r.duplicate, n, np.uint8), "scored": arr(r.scored, n, np.uint8), "score_q": arr(r.score_q, n, np.int32),
                    "rescaled": arr(r.rescaled_quals, int(r.n_quals), np.uint8)}
        finally:
            lib().mapad_aln_result_free(out)

    def alignment_tracks(self):
        """mapad_ctx_alignment_tracks: the arrays the device built for the batch accumulated last (the dict alignment_tracks_host returns)"""
        out = C.POINTER(TracksC)()
        _check(lib().mapad_ctx_alignment_tracks(self.h, C.byref(out)), "mapad_ctx_alignment_tracks")
        return _tracks_dict(out)

    def map_batch(self, seqs, quals, offsets):
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        out = C.POINTER(BatchResultC)()
        _check(lib().mapad_map_batch(self.h, _ptr(seqs), _ptr(quals), _ptr(offsets), offsets.size - 1, C.byref(out)), "mapad_map_batch")
        return BatchResult(out, lib().mapad_batch_result_free)

    def submit_batch(self, seqs, quals, offsets):
        """asynchronous map_batch: returns once the reads are staged and the kernels are enqueued (collect with select_batch + fetch)"""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        _check(lib().mapad_submit_batch(self.h, _ptr(seqs), _ptr(quals), _ptr(offsets), offsets.size - 1), "mapad_submit_batch")

    def map_batch_device(self, d_seqs, d_quals, d_offsets, n_reads, max_read_len):
        _check(lib().mapad_map_batch_device(self.h, d_seqs, d_quals, d_offsets, n_reads, max_read_len), "mapad_map_batch_device")

    def fetch(self):
        out = C.POINTER(BatchResultC)()
        _check(lib().mapad_fetch_result(self.h, C.byref(out)), "mapad_fetch_result")
        return BatchResult(out, lib().mapad_batch_result_free)

    def set_pipeline_depth(self, depth):
        _check(lib().mapad_ctx_set_pipeline_depth(self.h, int(depth)), "mapad_ctx_set_pipeline_depth")

    def reserve(self, n_reads, total_bases, max_read_len, host_inputs=False):
        _check(lib().mapad_ctx_reserve(self.h, int(n_reads), int(total_bases), int(max_read_len), int(host_inputs)), "mapad_ctx_reserve")

    def select_batch(self, age):
        _check(lib().mapad_ctx_select_batch(self.h, int(age)), "mapad_ctx_select_batch")

    def kernel_history(self, cap=4096):
        """(n_launches, 4) float32: ms from the first launch's start to each launch's four event marks; clears the history"""
        out = np.zeros((cap, 4), np.float32)
        n = C.c_uint32()
        _check(lib().mapad_kernel_history(self.h, _ptr(out), cap, C.byref(n)), "mapad_kernel_history")
        return out[:min(cap, int(n.value))].copy()

    def records_device(self, seed=0):
        """record fields of the selected batch on the device: (d_records [n x 88 B], d_text, d_pairs, text_bytes, n_pairs) — what the multi-GPU gather sends"""
        p = [C.c_void_p() for _ in range(3)]
        nt, npairs = _u64(), _u64()
        _check(lib().mapad_records_device(self.h, int(seed), C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(nt), C.byref(npairs)), "mapad_records_device")
        return p[0].value, p[1].value, p[2].value, int(nt.value), int(npairs.value)

    def compact_device(self):
        """device-side order-preserving collect of the last batch: (d_hit_begin, d_hits, d_ops, n_hits, n_ops)"""
        p = [C.c_void_p() for _ in range(3)]
        nh, no = C.c_uint64(), C.c_uint64()
        _check(lib().mapad_compact_result_device(self.h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(nh), C.byref(no)), "mapad_compact_result_device")
        return p[0].value, p[1].value, p[2].value, int(nh.value), int(no.value)

    def device_result_ptrs(self):
        p = [C.c_void_p() for _ in range(5)]
        _check(lib().mapad_device_result_ptrs(self.h, *[C.byref(x) for x in p]), "mapad_device_result_ptrs")
        return [x.value for x in p]

    def last_counters(self):
        out = np.zeros(6, np.uint64)
        _check(lib().mapad_last_batch_counters(self.h, _ptr(out)), "mapad_last_batch_counters")
        return out

    def kernel_ms(self):
        """HIP-event durations (ms) of the last batch: (D arrays + ordering, search over every read + retries, full-limit search)"""
        out = np.zeros(3, np.float32)
        _check(lib().mapad_last_kernel_ms(self.h, _ptr(out)), "mapad_last_kernel_ms")
        return out

    def set_reserved_cus(self, n):
        """Leave the last n CUs free of this context's launches (room for RCCL's transfer kernels beside a search; before the first batch, depth >= 2)."""
        _check(lib().mapad_ctx_set_reserved_cus(self.h, int(n)), "mapad_ctx_set_reserved_cus")

    def set_tail_pops(self, pops):
        """Pop budget of a read on the GPU before the library's host threads take it over (0 = never; csrc/host_tail.hpp)."""
        _check(lib().mapad_ctx_set_tail_pops(self.h, int(pops)), "mapad_ctx_set_tail_pops")

    def tail_info(self):
        """{reads, gpu_pops, host_pops, host_us (wall), threads, budget, ..., host_thread_us (summed over the threads)} of the selected batch's host tail (after its collect / fetch)."""
        out = np.zeros(16, np.uint64)
        _check(lib().mapad_last_tail_info(self.h, _ptr(out)), "mapad_last_tail_info")
        d = dict(zip(("reads", "gpu_pops", "host_pops", "host_us", "threads", "budget", "host_e_search", "host_n_push", "host_n_node", "host_thread_us",
                      "seen_live", "reads_dry_class", "reads_full_limit", "min_class", "continued", "handed_over_with_state"), (int(x) for x in out)))
        d["reads_idle_tier"] = d["min_class"] >> 32  # word 13: dry-class threshold | reads handed over below the budget because a worker was idle << 32
        d["min_class"] &= 0xFFFFFFFF
        return d

    def launch_info(self):
        out = np.zeros(8, np.uint32)
        _check(lib().mapad_last_launch_info(self.h, _ptr(out)), "mapad_last_launch_info")
        return out

    def sa_locate(self, rows):
        """Suffix-array values of BWT rows, located by the device kernel (UINT64_MAX for rows past the text)."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        out = np.zeros(rows.size, np.uint64)
        _check(lib().mapad_sa_locate(self.h, _ptr(rows) if rows.size else None, rows.size, _ptr(out) if rows.size else None), "mapad_sa_locate")
        return out

    def locate_info(self):
        ms, rows, steps = C.c_float(), C.c_uint64(), C.c_uint64()
        _check(lib().mapad_last_locate_info(self.h, C.byref(ms), C.byref(rows), C.byref(steps)), "mapad_last_locate_info")
        return float(ms.value), int(rows.value), int(steps.value)

    def hits_to_records(self, result_cptr_owner, seqs, quals, offsets, in_flags=None, seed=0, as_arrays=False, *, rescaled=False):
        """mapad_hits_to_records_gpu -> list of dicts, same as hits_to_records() with the SA lookups done on the device.  as_arrays: (records as a numpy structured
        array with RecordC's fields, text bytes) instead — for millions of reads; with the damage score on: (records, text, score_q int32, scored uint8).
        rescaled=True appends the batch's rescaled qualities (uint8, at `offsets`; None while the quality rescaling is off) as the last element: of the tuple
        with as_arrays, of (list of dicts, rescaled) without."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        fl = None if in_flags is None else np.ascontiguousarray(in_flags, dtype=np.uint16)
        out = C.POINTER(RecordsC)()
        _check(lib().mapad_hits_to_records_gpu(self.h, result_cptr_owner._cptr, _ptr(seqs), _ptr(quals), _ptr(offsets),
                                               _ptr(fl) if fl is not None else None, seed, C.byref(out)), "mapad_hits_to_records_gpu")
        if not rescaled:
            return _records_arrays(out) if as_arrays else _decode_records(out)
        rq = _records_rescaled(out)  # (copied: the decoders below free `out`)
        return _records_arrays(out) + (rq,) if as_arrays else (_decode_records(out), rq)


_CIGAR_OPS = {c: i for i, c in enumerate("MIDNSHP=X")}


def pack_alignments(records):
    """records: dicts with "tid", "pos" (0-based), "cigar" (text), "md" (text, None = no MD) and optionally "flags" (or "mapped" / "reverse"), "mapq", "x0" (None =
    no X0 tag), "as" -> (alns: ALIGNMENT_DTYPE[n], cigar_words uint32, md_bytes uint8), the three arrays accumulate_alignments and alignment_tracks_host take"""
    alns = np.zeros(len(records), ALIGNMENT_DTYPE)
    words, md = [], bytearray()
    for i, r in enumerate(records):
        flags = r.get("flags")
        if flags is None:
            flags = (0 if r.get("mapped", True) else 0x4) | (0x10 if r.get("reverse") else 0)
        a = alns[i]
        a["tid"], a["pos0"], a["flags"], a["mapq"] = r.get("tid", -1), r.get("pos", -1), flags & 0xFFFF, r.get("mapq", 0)
        a["x0"], a["as_score"] = r.get("x0") or 0, r.get("as") or 0.0
        a["cigar_off"], a["md_off"] = len(words), len(md)
        num = ""
        for ch in r.get("cigar") or "":
            if ch.isdigit():
                num += ch
            else:
                words.append(int(num) << 4 | _CIGAR_OPS[ch])
                num = ""
        a["n_cigar"] = len(words) - int(a["cigar_off"])
        md += (r.get("md") or "").encode()
        a["md_len"] = len(md) - int(a["md_off"])
    return alns, np.array(words, np.uint32), np.frombuffer(bytes(md), np.uint8)


def _alignment_arrays(alns, cigar_words, md_bytes, n):
    alns = np.ascontiguousarray(alns, dtype=ALIGNMENT_DTYPE)
    if alns.size != n:
        raise ValueError("one alignment per read")
    cigar_words = np.ascontiguousarray(cigar_words, dtype=np.uint32)
    md_bytes = np.ascontiguousarray(md_bytes, dtype=np.uint8)
    if n and (int((alns["cigar_off"] + alns["n_cigar"]).max()) > cigar_words.size or int((alns["md_off"] + alns["md_len"]).max()) > md_bytes.size):
        raise ValueError("an alignment points beyond cigar_words / md_bytes")
    # (an empty array has no address worth passing: one spare element keeps the pointers non-NULL)
    return alns, (cigar_words if cigar_words.size else np.zeros(1, np.uint32)), (md_bytes if md_bytes.size else np.zeros(1, np.uint8))


def _tracks_dict(out):
    """mapad_tracks_t -> dict of copied numpy arrays; frees the C object"""
    try:
        t = out.contents
        n, n_ops = int(t.n_reads), int(t.n_ops)

        def arr(p, count, dtype):
            return np.frombuffer(C.string_at(p, count * np.dtype(dtype).itemsize), dtype).copy() if count else np.zeros(0, dtype)

        d = {"hit_begin": arr(t.hit_begin, n + 1, np.uint64), "hits": arr(t.hits, n, HIT_DTYPE), "ops": arr(t.ops, n_ops, np.uint32),
             "status_class": arr(t.status_class, n, np.uint8), "class_counts": {k: int(t.class_counts[i]) for i, k in enumerate(ALN_CLASSES)}}
        for k, dt in (("mapped", np.uint32), ("error", np.uint32), ("best", np.uint32), ("x0", np.uint64), ("tid", np.int32), ("rel", np.uint64), ("abs", np.uint64),
                      ("backward", np.uint32)):
            d[k] = arr(getattr(t, k), n, dt)
        return d
    finally:
        lib().mapad_tracks_free(out)


def alignment_tracks_host(index, params, offsets, alns, cigar_words, md_bytes, min_mapq=0):
    """mapad_alignment_tracks_host: the tracks of alignments built on the CPU with align_core.hpp (no GPU) -> {"hit_begin", "hits" (HIT_DTYPE), "ops",
    "status_class", "class_counts", and the CoordRec fields "mapped", "error", "best", "x0", "tid", "rel", "abs", "backward"}"""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    alns, cigar_words, md_bytes = _alignment_arrays(alns, cigar_words, md_bytes, offsets.size - 1)
    out = C.POINTER(TracksC)()
    _check(lib().mapad_alignment_tracks_host(index.h, C.byref(params), _ptr(offsets), offsets.size - 1, _ptr(alns), _ptr(cigar_words), _ptr(md_bytes), int(min_mapq),
                                             C.byref(out)), "mapad_alignment_tracks_host")
    return _tracks_dict(out)


def _damage_dict(c):
    d = {"counts": np.ctypeslib.as_array(c.counts).astype(np.uint64).reshape(2, DAMAGE_POSITIONS, 4, 4).copy()}
    for k in ("reads", "reads_seen", "aligned_bases", "skipped_bases", "insertions", "deletions", "batches"):
        d[k] = int(getattr(c, k))
    d["kernel_ms"] = float(c.kernel_ms)
    return d


def _damage_scores_dict(c):
    d = {k: int(getattr(c, k)) for k in ("reads_seen", "reads_scored", "reads_below", "informative_columns", "score_sum", "batches", "threshold_q")}
    d["histogram"] = np.ctypeslib.as_array(c.histogram).astype(np.uint64).copy()
    d["kernel_ms"] = float(c.kernel_ms)
    return d


def damage_score_host(index, params, result_cptr_owner, seqs, quals, offsets, seed=0, threshold=0.0, into=None):
    """mapad_damage_score_host: the damage scores of one result computed on the host (no GPU), the reported hit chosen as hits_to_records(seed=seed) chooses it.
    Returns (score_q int32[n] in 1/256 bit, scored uint8[n], summary as Context.damage_scores() returns it); `into`: a summary returned earlier, to which this
    batch is added."""
    seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
    quals = np.ascontiguousarray(quals, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = offsets.size - 1
    score_q, scored = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    acc = DamageScoresC()
    _check(lib().mapad_damage_score_host(index.h, C.byref(params), result_cptr_owner._cptr, _ptr(seqs), _ptr(quals), _ptr(offsets), int(seed), float(threshold),
                                         _ptr(score_q) if n else None, _ptr(scored) if n else None, C.byref(acc)), "mapad_damage_score_host")
    d = _damage_scores_dict(acc)
    if into is not None:
        for k in d:
            if k != "threshold_q":
                d[k] = into[k] + d[k]
    return score_q, scored, d


def _rescale_dict(c):
    d = {k: int(getattr(c, k)) for k in ("reads_seen", "reads_rescaled", "bases_changed", "quality_drop_sum", "batches")}
    d["candidate_columns"] = np.ctypeslib.as_array(c.candidate_columns).astype(np.uint64).copy()
    d["new_quality"] = np.ctypeslib.as_array(c.new_quality).astype(np.uint64).copy()
    d["kernel_ms"] = float(c.kernel_ms)
    return d


def quality_rescale_host(index, params, result_cptr_owner, seqs, quals, offsets, seed=0, into=None):
    """mapad_quality_rescale_host: the rescaled qualities of one result computed on the host (no GPU), the reported hit chosen as hits_to_records(seed=seed)
    chooses it.  Returns (rescaled uint8, at `offsets`; summary as Context.quality_rescale() returns it); `into`: a summary returned earlier, to which this batch
    is added."""
    seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
    quals = np.ascontiguousarray(quals, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = offsets.size - 1
    out = np.zeros(int(offsets[n]) if n else 0, np.uint8)
    acc = RescaleC()
    _check(lib().mapad_quality_rescale_host(index.h, C.byref(params), result_cptr_owner._cptr, _ptr(seqs), _ptr(quals), _ptr(offsets), int(seed),
                                            _ptr(out) if out.size else None, C.byref(acc)), "mapad_quality_rescale_host")
    d = _rescale_dict(acc)
    if into is not None:
        for k in d:
            d[k] = into[k] + d[k]
    return out, d


def quality_rescale_table(params, length):
    """mapad_quality_rescale_table: one read length's table as the device gets it, uint8[length, 256, 2] — the new quality byte of a C->T (0) / G->A (1)
    mismatch by read position and quality byte; the row of the missing quality 255 holds 255."""
    out = np.zeros((int(length), 256, 2), np.uint8)
    _check(lib().mapad_quality_rescale_table(C.byref(params), int(length), _ptr(out)), "mapad_quality_rescale_table")
    return out


def damage_score_table(params, length):
    """mapad_damage_score_table: one read length's table as the device gets it, int16[length, nq, 4] in 1/256 bit — C->C, C->T, G->G, G->A (reference base -> read
    base, read orientation); nq = 256 quality levels for the quality-aware model, else 1."""
    nq = C.c_int()
    _check(lib().mapad_damage_score_table(C.byref(params), int(length), None, C.byref(nq)), "mapad_damage_score_table")
    out = np.zeros((int(length), int(nq.value), 4), np.int16)
    _check(lib().mapad_damage_score_table(C.byref(params), int(length), _ptr(out), C.byref(nq)), "mapad_damage_score_table")
    return out


def _duplicates_dict(c):
    d = {k: int(getattr(c, k)) for k in ("reads_seen", "reads_eligible", "duplicates", "fragments", "slots", "grows", "batches")}
    d["histogram"] = np.ctypeslib.as_array(c.histogram).astype(np.uint64).copy()
    d["mark_ms"], d["summary_ms"] = float(c.mark_ms), float(c.summary_ms)
    return d


def _skip_ptr(skip, n):
    """a per-read skip array (1 = leave the read out) as (kept-alive uint8 array, pointer); None -> NULL"""
    if skip is None:
        return None, None
    a = np.ascontiguousarray(skip, dtype=np.uint8)
    if a.size != n:
        raise ValueError("skip needs one entry per read")
    return a, _ptr(a)


class DedupHost:
    """mapad_dedup_host_*: PCR duplicates marked on the host (no GPU) over fetched results in the order in which they are added, the reported hit chosen as
    hits_to_records(seed=seed) chooses it.  add() returns the batch's flags (uint8, 1 = duplicate); summary() the same dict as Context.duplicates()."""

    def __init__(self):
        self.h = C.c_void_p()
        _check(lib().mapad_dedup_host_new(C.byref(self.h)), "mapad_dedup_host_new")

    def add(self, index, params, result_cptr_owner, seed=0):
        flags = np.zeros(int(result_cptr_owner.n_reads), np.uint8)
        _check(lib().mapad_dedup_host_add(self.h, index.h, C.byref(params), result_cptr_owner._cptr, int(seed), _ptr(flags) if flags.size else None), "mapad_dedup_host_add")
        return flags

    def summary(self):
        out = DuplicatesC()
        _check(lib().mapad_dedup_host_summary(self.h, C.byref(out)), "mapad_dedup_host_summary")
        return _duplicates_dict(out)

    def close(self):
        if self.h:
            lib().mapad_dedup_host_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def damage_profile_host(index, params, result_cptr_owner, seqs, offsets, seed=0, mode=1, into=None, skip=None):
    """mapad_damage_profile_host: the damage profile of one result computed on the host (no GPU), the reported hit chosen as hits_to_records(seed=seed) chooses it.
    Returns the same dict as Context.damage_profile(); `into`: a dict returned earlier, to which this batch is added; `skip`: uint8 per read, 1 = leave it out."""
    seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    acc = DamageProfileC()
    keep, sp = _skip_ptr(skip, offsets.size - 1)
    _check(lib().mapad_damage_profile_host_skip(index.h, C.byref(params), result_cptr_owner._cptr, _ptr(seqs), _ptr(offsets), int(seed), int(mode), sp, C.byref(acc)),
           "mapad_damage_profile_host")
    d = _damage_dict(acc)
    if into is not None:
        for k in d:
            d[k] = into[k] + d[k]
    return d


def _coverage_summary(index, call):
    names = [c[0] for c in index.contigs()]
    rows = (CoverageContigC * max(len(names), 1))()
    c = CoverageC()
    c.n_contigs, c.contigs = len(names), C.cast(rows, C.POINTER(CoverageContigC))
    call(C.byref(c))
    d = {"contigs": [dict({"name": names[t]}, **{k: int(getattr(rows[t], k)) for k, _ in CoverageContigC._fields_}) for t in range(int(c.n_contigs))],
         "hist": np.ctypeslib.as_array(c.hist).astype(np.uint64).copy()}
    for k in ("reads", "reads_seen", "covered_columns", "deleted_columns", "insertions", "batches"):
        d[k] = int(getattr(c, k))
    d["accumulate_ms"], d["summary_ms"] = float(c.accumulate_ms), float(c.summary_ms)
    return d


class CoverageHost:
    """mapad_coverage_host_*: depth of coverage accumulated on the host (no GPU) over fetched results, the reported hit chosen as hits_to_records(seed=seed) chooses
    it.  summary() returns the same dict as Context.coverage(), depth() the same array as Context.coverage_depth()."""

    def __init__(self, index, mode=1):
        self.index = index
        self.h = C.c_void_p()
        _check(lib().mapad_coverage_host_new(index.h, int(mode), C.byref(self.h)), "mapad_coverage_host_new")

    def add(self, params, result_cptr_owner, seed=0, skip=None):
        keep, sp = _skip_ptr(skip, int(result_cptr_owner.n_reads))
        _check(lib().mapad_coverage_host_add_skip(self.h, self.index.h, C.byref(params), result_cptr_owner._cptr, int(seed), sp), "mapad_coverage_host_add")
        return self

    def summary(self):
        return _coverage_summary(self.index, lambda out: _check(lib().mapad_coverage_host_summary(self.h, out), "mapad_coverage_host_summary"))

    def depth(self, tid, start, n):
        out = np.zeros(int(n), np.uint32)
        _check(lib().mapad_coverage_host_depth(self.h, int(tid), int(start), int(n), _ptr(out) if n else None), "mapad_coverage_host_depth")
        return out

    def close(self):
        if self.h:
            lib().mapad_coverage_host_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _seq_bytes(seq):
    return np.ascontiguousarray(np.frombuffer(seq, np.uint8) if isinstance(seq, (bytes, bytearray)) else np.asarray(seq, np.uint8))


def _mappability(call, what, tid, seq, start, n, k, e, verify, counts, cover):
    s = _seq_bytes(seq)
    n = s.size - int(start) if n is None else int(n)
    oc = np.zeros(max(n, 0), np.uint8) if counts else None
    ov = np.zeros(max(n, 0), np.uint8) if cover else None
    _check(call(int(tid), _ptr(s) if s.size else None, s.size, int(start), n, int(k), int(e), MAPPABILITY_VERIFY if verify else 0,
                _ptr(oc) if counts and n > 0 else None, _ptr(ov) if cover and n > 0 else None), what)
    return oc, ov


def _mappability_contig_dict(c):
    d = {k: int(getattr(c, k)) for k in ("length", "valid_starts", "unique_starts", "majority", "strict")}
    d["hist"] = [int(v) for v in c.hist]
    return d


def _mappability_summary(index, seqs, k, e, verify, call, what):
    names = [c[0] for c in index.contigs()]
    arrs = [_seq_bytes(s) for s in seqs]
    if len(arrs) != len(names):
        raise MapadError(-1, what + ": one sequence per contig of the index")
    ptrs = (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data if a.size else None for a in arrs])
    lens = (C.c_uint64 * max(len(arrs), 1))(*[a.size for a in arrs])
    rows = (MappabilityContigC * max(len(names), 1))()
    c = MappabilityC()
    c.n_contigs, c.contigs = len(names), C.cast(rows, C.POINTER(MappabilityContigC))
    _check(call(ptrs, lens, int(k), int(e), MAPPABILITY_VERIFY if verify else 0, C.byref(c)), what)
    return {"k": int(c.k), "e": int(c.e), "contigs": [dict({"name": names[t]}, **_mappability_contig_dict(rows[t])) for t in range(int(c.n_contigs))],
            "total": _mappability_contig_dict(c.total), "starts": int(c.starts), "steps": int(c.steps), "kernel_ms": float(c.kernel_ms)}


def mappability_host(index, tid, seq, start=0, n=None, k=35, e=0, verify=False, counts=True, cover=True):
    """Context.mappability on host threads, no GPU: the same bytes."""
    return _mappability(lambda *a: lib().mapad_mappability_host(index.h, *a), "mapad_mappability_host", tid, seq, start, n, k, e, verify, counts, cover)


def mappability_summary_host(index, seqs, k=35, e=0, verify=False):
    """Context.mappability_summary on host threads, no GPU: the same figures (kernel_ms 0)."""
    return _mappability_summary(index, seqs, k, e, verify, lambda *a: lib().mapad_mappability_summary_host(index.h, *a), "mapad_mappability_summary_host")


def snp_panel_rule(call="random", min_depth=1, transitions="keep", seed=0):
    """-> mapad_snp_panel_rule_t; call: "random" | "majority" (or 0 | 1), transitions: "keep" | "missing" | "single_strand" (or 0 | 1 | 2)"""
    r = SnpPanelRuleC()
    r.call, r.min_depth = int(SNP_PANEL_CALLS.get(call, call)), int(min_depth)
    r.transitions, r.seed = int(SNP_PANEL_TRANSITIONS.get(transitions, transitions)), int(seed) & 0xFFFFFFFFFFFFFFFF
    return r


def _panel_rows(tid, pos0, ref, alt):
    tid = np.ascontiguousarray(tid, dtype=np.int32)
    pos0 = np.ascontiguousarray(pos0, dtype=np.uint64)
    ref, alt = (np.frombuffer(bytes(a), np.uint8) if isinstance(a, (bytes, bytearray, str)) else np.ascontiguousarray(a, dtype=np.uint8) for a in
                ((ref.encode() if isinstance(ref, str) else ref), (alt.encode() if isinstance(alt, str) else alt)))
    if not (tid.ndim == pos0.ndim == ref.ndim == alt.ndim == 1 and tid.size == pos0.size == ref.size == alt.size):
        raise ValueError("tid, pos0, ref and alt take one entry per panel row")
    return tid, pos0, ref, alt


def _panel_summary(call, rule):
    c = SnpPanelC()
    r = snp_panel_rule(**(rule or {}))
    call(C.byref(r), C.byref(c))
    d = {k: int(getattr(c, k)) for k in ("mode", "min_base_quality", "mask5", "mask3", "n_rows", "n_slots", "batches") + SNP_PANEL_SCALARS + SNP_PANEL_WORDS}
    d["rule"] = {"call": int(c.rule.call), "min_depth": int(c.rule.min_depth), "transitions": int(c.rule.transitions), "seed": int(c.rule.seed)}
    d["accumulate_ms"], d["summary_ms"] = float(c.accumulate_ms), float(c.summary_ms)
    return d


class SnpPanelHost:
    """mapad_snp_panel_host_*: the SNP panel accumulated on the host (no GPU) over fetched results and the reads they are of, the reported hit chosen as
    hits_to_records(seed=seed) chooses it.  summary() returns the same dict as Context.snp_panel(), counts() / calls() the same arrays as
    Context.snp_panel_counts() / Context.snp_panel_calls()."""

    def __init__(self, index, mode, tid, pos0, ref, alt, min_bq=0, mask5=0, mask3=0):
        self.index = index
        self.h = C.c_void_p()
        keep = _panel_rows(tid, pos0, ref, alt)
        _check(lib().mapad_snp_panel_host_new(index.h, int(mode), keep[0].size, *(_ptr(a) for a in keep), int(min_bq), int(mask5), int(mask3), C.byref(self.h)),
               "mapad_snp_panel_host_new")

    def add(self, params, result_cptr_owner, seqs, quals, offsets, seed=0, skip=None):
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        keep, sp = _skip_ptr(skip, offsets.size - 1)
        _check(lib().mapad_snp_panel_host_add_skip(self.h, self.index.h, C.byref(params), result_cptr_owner._cptr, _ptr(seqs), _ptr(quals), _ptr(offsets), int(seed), sp),
               "mapad_snp_panel_host_add")
        return self

    def summary(self, rule=None):
        return _panel_summary(lambda r, out: _check(lib().mapad_snp_panel_host_summary(self.h, r, out), "mapad_snp_panel_host_summary"), rule)

    def counts(self, row_from, n):
        out = np.zeros((int(n), 2, 4), np.uint32)
        _check(lib().mapad_snp_panel_host_counts(self.h, int(row_from), int(n), _ptr(out) if n else None), "mapad_snp_panel_host_counts")
        return out

    def calls(self, row_from, n, rule=None):
        out = np.zeros(int(n), np.uint8)
        r = snp_panel_rule(**(rule or {}))
        _check(lib().mapad_snp_panel_host_calls(self.h, int(row_from), int(n), C.byref(r), _ptr(out) if n else None), "mapad_snp_panel_host_calls")
        return out

    def close(self):
        if self.h:
            lib().mapad_snp_panel_host_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _pileup_summary(index, call):
    names = [c[0] for c in index.contigs()]
    rows = (PileupContigC * max(len(names), 1))()
    c = PileupC()
    c.n_contigs, c.contigs = len(names), C.cast(rows, C.POINTER(PileupContigC))
    call(C.byref(c))
    d = {"contigs": [{"name": names[t], "length": int(rows[t].length), "sites_covered": int(rows[t].sites_covered), "sites_deep": int(rows[t].sites_deep),
                      "sites_called": int(rows[t].sites_called), "called": [int(x) for x in rows[t].called], "base_sum": [int(x) for x in rows[t].base_sum],
                      "max_depth": int(rows[t].max_depth)} for t in range(int(c.n_contigs))]}
    for k, _ in PileupC._fields_[3:-2]:
        d[k] = int(getattr(c, k))
    d["accumulate_ms"], d["summary_ms"] = float(c.accumulate_ms), float(c.summary_ms)
    return d


class PileupHost:
    """mapad_pileup_host_*: the pileup accumulated on the host (no GPU) over fetched results and the reads they are of, the reported hit chosen as
    hits_to_records(seed=seed) chooses it.  summary() returns the same dict as Context.pileup(), counts() / consensus() the same arrays as
    Context.pileup_counts() / Context.pileup_consensus()."""

    def __init__(self, index, mode=1, min_bq=0, mask5=0, mask3=0):
        self.index = index
        self.h = C.c_void_p()
        _check(lib().mapad_pileup_host_new(index.h, int(mode), int(min_bq), int(mask5), int(mask3), C.byref(self.h)), "mapad_pileup_host_new")

    def add(self, params, result_cptr_owner, seqs, quals, offsets, seed=0, skip=None):
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        keep, sp = _skip_ptr(skip, offsets.size - 1)
        _check(lib().mapad_pileup_host_add_skip(self.h, self.index.h, C.byref(params), result_cptr_owner._cptr, _ptr(seqs), _ptr(quals), _ptr(offsets), int(seed), sp),
               "mapad_pileup_host_add")
        return self

    def summary(self, min_depth=1, min_percent=0):
        return _pileup_summary(self.index, lambda out: _check(lib().mapad_pileup_host_summary(self.h, int(min_depth), int(min_percent), out), "mapad_pileup_host_summary"))

    def counts(self, tid, start, n):
        out = np.zeros((int(n), 4), np.uint32)
        _check(lib().mapad_pileup_host_counts(self.h, int(tid), int(start), int(n), _ptr(out) if n else None), "mapad_pileup_host_counts")
        return out

    def consensus(self, tid, start, n, min_depth=1, min_percent=0):
        out = np.zeros(int(n), np.uint8)
        _check(lib().mapad_pileup_host_consensus(self.h, int(tid), int(start), int(n), int(min_depth), int(min_percent), _ptr(out) if n else None),
               "mapad_pileup_host_consensus")
        return out

    def close(self):
        if self.h:
            lib().mapad_pileup_host_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _allele_summary(index, call):
    names = [c[0] for c in index.contigs()]
    rows = (AlleleContigC * max(len(names), 1))()
    c = AlleleC()
    c.n_contigs, c.contigs = len(names), C.cast(rows, C.POINTER(AlleleContigC))
    call(C.byref(c))
    d = {"contigs": [{"name": names[t], "length": int(rows[t].length), "sites_covered": int(rows[t].sites_covered), "sites_deep": int(rows[t].sites_deep),
                      "sites_called": int(rows[t].sites_called), "called": [int(x) for x in rows[t].called], "max_depth": int(rows[t].max_depth),
                      "margin_sum_q": int(rows[t].margin_sum_q)} for t in range(int(c.n_contigs))]}
    for k, _ in AlleleC._fields_[3:-2]:
        d[k] = int(getattr(c, k))
    d["accumulate_ms"], d["summary_ms"] = float(c.accumulate_ms), float(c.summary_ms)
    return d


def _genotype_summary(index, call):
    names = [c[0] for c in index.contigs()]
    rows = (GenotypeContigC * max(len(names), 1))()
    c = GenotypeC()
    c.n_contigs, c.contigs = len(names), C.cast(rows, C.POINTER(GenotypeContigC))
    call(C.byref(c))
    d = {"contigs": [{"name": names[t], "length": int(rows[t].length), "sites_covered": int(rows[t].sites_covered), "sites_deep": int(rows[t].sites_deep),
                      "sites_called": int(rows[t].sites_called), "called": [int(x) for x in rows[t].called], "max_depth": int(rows[t].max_depth),
                      "margin_sum_q": int(rows[t].margin_sum_q)} for t in range(int(c.n_contigs))]}
    for k in ("on", "min_depth", "min_margin_q", "het_penalty_q", "batches"):
        d[k] = int(getattr(c, k))
    d["accumulate_ms"], d["summary_ms"] = float(c.accumulate_ms), float(c.summary_ms)
    return d


class AlleleHost:
    """mapad_allele_host_*: the allele likelihoods accumulated on the host (no GPU) over fetched results and the reads they are of, the reported hit chosen as
    hits_to_records(seed=seed) chooses it.  summary() returns the same dict as Context.allele_summary(), cells() / consensus() the same arrays as
    Context.allele_cells() / Context.allele_consensus()."""

    def __init__(self, index, mode=1, min_bq=0, mask5=0, mask3=0, genotypes=False):
        self.index = index
        self.h = C.c_void_p()
        _check(lib().mapad_allele_host_new(index.h, int(mode), int(min_bq), int(mask5), int(mask3), C.byref(self.h)), "mapad_allele_host_new")
        if genotypes:  # the het cells beside the allele cells: genotype_summary() / genotype_cells() / genotype_calls() as on a Context
            _check(lib().mapad_allele_host_set_genotypes(self.h, 1), "mapad_allele_host_set_genotypes")

    def genotype_summary(self, min_depth=1, min_margin=3.0, het_penalty=0.0):
        return _genotype_summary(self.index, lambda out: _check(lib().mapad_allele_host_genotype_summary(self.h, int(min_depth), float(min_margin), float(het_penalty), out),
                                                                "mapad_allele_host_genotype_summary"))

    def genotype_cells(self, tid, start, n):
        het = np.zeros((int(n), 6), np.int32)
        _check(lib().mapad_allele_host_genotype_cells(self.h, int(tid), int(start), int(n), _ptr(het) if n else None), "mapad_allele_host_genotype_cells")
        return het

    def genotype_calls(self, tid, start, n, min_depth=1, min_margin=3.0, het_penalty=0.0):
        gt, gq = np.zeros(int(n), np.uint8), np.zeros(int(n), np.uint8)
        _check(lib().mapad_allele_host_genotype_calls(self.h, int(tid), int(start), int(n), int(min_depth), float(min_margin), float(het_penalty),
                                                      _ptr(gt) if n else None, _ptr(gq) if n else None), "mapad_allele_host_genotype_calls")
        return gt, gq

    def add(self, params, result_cptr_owner, seqs, quals, offsets, seed=0, skip=None):
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        keep, sp = _skip_ptr(skip, offsets.size - 1)
        _check(lib().mapad_allele_host_add_skip(self.h, self.index.h, C.byref(params), result_cptr_owner._cptr, _ptr(seqs), _ptr(quals), _ptr(offsets), int(seed), sp),
               "mapad_allele_host_add")
        return self

    def summary(self, min_depth=1, min_margin=3.0):
        return _allele_summary(self.index, lambda out: _check(lib().mapad_allele_host_summary(self.h, int(min_depth), float(min_margin), out), "mapad_allele_host_summary"))

    def cells(self, tid, start, n):
        ll, depth = np.zeros((int(n), 4), np.int32), np.zeros(int(n), np.uint32)
        _check(lib().mapad_allele_host_cells(self.h, int(tid), int(start), int(n), _ptr(ll) if n else None, _ptr(depth) if n else None), "mapad_allele_host_cells")
        return ll, depth

    def consensus(self, tid, start, n, min_depth=1, min_margin=3.0):
        bases, quals = np.zeros(int(n), np.uint8), np.zeros(int(n), np.uint8)
        _check(lib().mapad_allele_host_consensus(self.h, int(tid), int(start), int(n), int(min_depth), float(min_margin), _ptr(bases) if n else None,
                                                 _ptr(quals) if n else None), "mapad_allele_host_consensus")
        return bases, quals

    def close(self):
        if self.h:
            lib().mapad_allele_host_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def allele_quantized_row(params, length, pos, qual, to):
    """mapad_allele_quantized_row: int16[4], what a counted column of read base `to` (0..3 = A, C, G, T, read orientation) at read position `pos` of a read of
    `length` bases with raw Phred `qual` adds by true base A, C, G, T in read orientation, in 1/256 bit"""
    out = np.zeros(4, np.int16)
    _check(lib().mapad_allele_quantized_row(C.byref(params), int(length), int(pos), int(qual), int(to), _ptr(out)), "mapad_allele_quantized_row")
    return out


def genotype_quantized_row(params, length, pos, qual, to):
    """mapad_genotype_quantized_row: int16[6], what a counted column of read base `to` (0..3 = A, C, G, T, read orientation) at read position `pos` of a read
    of `length` bases with raw Phred `qual` adds by pair of true bases AC AG AT CG CT GT in read orientation, in 1/256 bit"""
    out = np.zeros(6, np.int16)
    _check(lib().mapad_genotype_quantized_row(C.byref(params), int(length), int(pos), int(qual), int(to), _ptr(out)), "mapad_genotype_quantized_row")
    return out


def _records_arrays(out):
    """mapad_records_t -> (records as a numpy structured array with RecordC's fields, text bytes as uint8), copied; frees the C object"""
    r = out.contents
    n = int(r.n)
    recs = np.frombuffer(C.string_at(C.addressof(r.recs.contents), n * C.sizeof(RecordC)), np.dtype(RecordC)).copy() if n else np.zeros(0, np.dtype(RecordC))
    text = np.frombuffer(C.string_at(r.text, r.text_len), np.uint8).copy() if r.text_len else np.zeros(0, np.uint8)
    scores = _records_scores(out, n)
    lib().mapad_records_free(out)
    return (recs, text) if scores is None else (recs, text) + scores


def hits_to_records(index, params, result_cptr_owner, seqs, quals, offsets, in_flags=None, seed=0, as_arrays=False):
    """mapad_hits_to_records -> list of dicts (decoded record fields); as_arrays: (records structured array, text bytes)."""
    seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
    quals = np.ascontiguousarray(quals, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    fl = None if in_flags is None else np.ascontiguousarray(in_flags, dtype=np.uint16)
    out = C.POINTER(RecordsC)()
    _check(lib().mapad_hits_to_records(index.h, C.byref(params), result_cptr_owner._cptr, _ptr(seqs), _ptr(quals), _ptr(offsets),
                                       _ptr(fl) if fl is not None else None, seed, C.byref(out)), "mapad_hits_to_records")
    return _records_arrays(out) if as_arrays else _decode_records(out)


def _records_scores(out, n):
    """the damage scores that travel beside a mapad_records_t: (score_q int32[n], scored uint8[n]) copied, or None when the records carry none"""
    sq, sc = C.c_void_p(), C.c_void_p()
    _check(lib().mapad_records_damage_scores(out, C.byref(sq), C.byref(sc)), "mapad_records_damage_scores")
    if not sq.value or not sc.value:
        return None
    return np.frombuffer(C.string_at(sq.value, 4 * n), np.int32).copy(), np.frombuffer(C.string_at(sc.value, n), np.uint8).copy()


def _records_rescaled(out):
    """the rescaled qualities that travel beside a mapad_records_t, copied, or None when the records carry none"""
    q, n = C.c_void_p(), C.c_uint64()
    _check(lib().mapad_records_rescaled_quals(out, C.byref(q), C.byref(n)), "mapad_records_rescaled_quals")
    if not q.value:
        return None
    return np.frombuffer(C.string_at(q.value, int(n.value)), np.uint8).copy()


def _decode_records(out):
    r = out.contents
    text = C.string_at(r.text, r.text_len)
    recs = []
    scores = _records_scores(out, int(r.n))
    for i in range(r.n):
        c = r.recs[i]
        recs.append({"flags": c.flags, "duplicate": bool(c.flags & 0x400), "mapq": c.mapq, "mapped": bool(c.mapped), "reverse": bool(c.reverse), "tid": c.tid, "pos": c.pos,
                     "as": np.float32(c.as_score), "xs": np.float32(c.xs_score) if c.has_xs else None, "nm": c.nm, "x0": c.x0, "x1": c.x1,
                     "xt": c.xt.decode() if c.mapped else None,
                     "cigar": text[c.cigar_off:c.cigar_off + c.cigar_len].decode(), "md": text[c.md_off:c.md_off + c.md_len].decode(),
                     "xa": text[c.xa_off:c.xa_off + c.xa_len].decode()})
        if scores is not None:  # the context's damage score is on: bits, None for a read without a score
            recs[-1]["damage_score"] = float(scores[0][i]) / 256.0 if scores[1][i] else None
    lib().mapad_records_free(out)
    return recs


# ---- adapter trimming and read-pair merging (include/mapad_amd.h: mapad_merger_t; DESIGN.md section 4 "Trim and merge") --------------------------------------
def merge_params(mode=0, adapter1=None, adapter2=None, **kw):
    """mapad_merge_params_t: the defaults, then min_overlap / min_adapter_overlap / max_mismatch_permille / min_length / max_quality and the adapters as given;
    mode 0 = pairs, 1 = single-end.  Raises MapadError where mapad_merge_params_check refuses them."""
    p = MergeParamsC()
    lib().mapad_merge_params_default(C.byref(p))
    p.mode = int(mode)
    for name, seq in (("adapter1", adapter1), ("adapter2", adapter2)):
        if seq is None:
            continue
        seq = seq.encode() if isinstance(seq, str) else bytes(seq)
        setattr(p, name + "_len", len(seq))
        if len(seq) <= MERGE_MAX_ADAPTER:  # (a longer one is what the check below refuses)
            C.memset(getattr(p, name), 0, MERGE_MAX_ADAPTER)
            C.memmove(getattr(p, name), seq, len(seq))
    for k, v in kw.items():
        if k not in ("min_overlap", "min_adapter_overlap", "max_mismatch_permille", "min_length", "max_quality"):
            raise KeyError(k)
        setattr(p, k, int(v))
    _check(lib().mapad_merge_params_check(C.byref(p)), "mapad_merge_params_check")
    return p


def _merge_counts_dict(c):
    return {"pairs_seen": int(c.pairs_seen), "class_counts": np.array(c.class_counts[:], np.uint64), "bases_in": int(c.bases_in), "bases_out": int(c.bases_out),
            "histogram": np.array(c.histogram[:], np.uint64), "calls": int(c.calls)}


def _merge_result_dict(out):
    """copies a mapad_merge_result_t into numpy arrays and frees it"""
    r = out.contents
    n, total = int(r.n_pairs), int(r.total_bases)

    def arr(p, count, dtype):
        return np.frombuffer(C.string_at(p, count * np.dtype(dtype).itemsize), dtype).copy() if count else np.zeros(0, dtype)
    d = {"n_pairs": n, "cls": arr(r.cls, n, np.uint8), "frag_len": arr(r.frag_len, n, np.int32), "matches": arr(r.matches, n, np.uint16),
         "mismatches": arr(r.mismatches, n, np.uint16), "seqs": arr(r.seqs, total, np.uint8), "quals": arr(r.quals, total, np.uint8),
         "offsets": arr(r.offsets, n + 1, np.uint64), "counts": _merge_counts_dict(r.counts), "kernel_ms": (float(r.kernel_ms[0]), float(r.kernel_ms[1]))}
    lib().mapad_merge_result_free(out)
    return d


def _packed(seqs, quals, offsets):
    return np.ascontiguousarray(seqs, dtype=np.uint8), np.ascontiguousarray(quals, dtype=np.uint8), np.ascontiguousarray(offsets, dtype=np.uint64)


def merge_pairs_host(params, seqs1, quals1, offsets1, seqs2, quals2, offsets2):
    """the merge rule on host threads, no GPU (params: merge_params(mode=0))"""
    s1, q1, o1 = _packed(seqs1, quals1, offsets1)
    s2, q2, o2 = _packed(seqs2, quals2, offsets2)
    out = C.POINTER(MergeResultC)()
    _check(lib().mapad_merge_pairs_host(C.byref(params), _ptr(s1), _ptr(q1), _ptr(o1), _ptr(s2), _ptr(q2), _ptr(o2), o1.size - 1, C.byref(out)), "mapad_merge_pairs_host")
    return _merge_result_dict(out)


def trim_reads_host(params, seqs, quals, offsets):
    """single-end trimming on host threads, no GPU (params: merge_params(mode=1))"""
    s, q, o = _packed(seqs, quals, offsets)
    out = C.POINTER(MergeResultC)()
    _check(lib().mapad_trim_reads_host(C.byref(params), _ptr(s), _ptr(q), _ptr(o), o.size - 1, C.byref(out)), "mapad_trim_reads_host")
    return _merge_result_dict(out)


class Merger:
    """mapad_merger_t: the trim-and-merge stage on one device.  It needs no index and no Context."""

    def __init__(self, params, device_id=0):
        self.h = C.c_void_p()
        self.params = params
        _check(lib().mapad_merger_create(int(device_id), C.byref(params), C.byref(self.h)), "mapad_merger_create")

    def set_stream(self, stream_ptr):
        _check(lib().mapad_merger_set_stream(self.h, C.c_void_p(stream_ptr)), "mapad_merger_set_stream")

    def merge_pairs(self, seqs1, quals1, offsets1, seqs2, quals2, offsets2):
        s1, q1, o1 = _packed(seqs1, quals1, offsets1)
        s2, q2, o2 = _packed(seqs2, quals2, offsets2)
        out = C.POINTER(MergeResultC)()
        _check(lib().mapad_merge_pairs(self.h, _ptr(s1), _ptr(q1), _ptr(o1), _ptr(s2), _ptr(q2), _ptr(o2), o1.size - 1, C.byref(out)), "mapad_merge_pairs")
        return _merge_result_dict(out)

    def trim_reads(self, seqs, quals, offsets):
        s, q, o = _packed(seqs, quals, offsets)
        out = C.POINTER(MergeResultC)()
        _check(lib().mapad_trim_reads(self.h, _ptr(s), _ptr(q), _ptr(o), o.size - 1, C.byref(out)), "mapad_trim_reads")
        return _merge_result_dict(out)

    def merge_pairs_device(self, d_seqs1, d_quals1, d_offsets1, d_seqs2, d_quals2, d_offsets2, n_pairs):
        """device pointers in, (d_seqs, d_quals, d_offsets, total_bases) out: the merger's own buffers, valid until its next call"""
        p = [C.c_void_p() for _ in range(3)]
        total = _u64()
        _check(lib().mapad_merge_pairs_device(self.h, d_seqs1, d_quals1, d_offsets1, d_seqs2, d_quals2, d_offsets2, int(n_pairs), C.byref(p[0]), C.byref(p[1]), C.byref(p[2]),
                                              C.byref(total)), "mapad_merge_pairs_device")
        return p[0].value, p[1].value, p[2].value, int(total.value)

    def totals(self):
        c = MergeCountsC()
        _check(lib().mapad_merger_totals(self.h, C.byref(c)), "mapad_merger_totals")
        return _merge_counts_dict(c)

    def reset(self):
        _check(lib().mapad_merger_reset(self.h), "mapad_merger_reset")

    def close(self):
        if self.h:
            lib().mapad_merger_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- read clean-up (include/mapad_amd.h: mapad_cleaner_t; DESIGN.md section 4 "Clean") ---------------------------------------------------------------------------
def clean_params(ops=0, **kw):
    """mapad_clean_params_t: the defaults, then poly_base / poly_min_len / poly_one_in / poly_max_mismatch / min_quality / min_length / max_dust as given.  `ops`: a
    mask, or names of CLEAN_OPS ("poly", "trim_n", "trim_qual", "dust").  Raises MapadError where mapad_clean_params_check refuses them."""
    p = CleanParamsC()
    lib().mapad_clean_params_default(C.byref(p))
    p.ops = int(ops) if isinstance(ops, (int, np.integer)) else sum(CLEAN_OPS[o] for o in ops)
    for k, v in kw.items():
        if k not in ("poly_base", "poly_min_len", "poly_one_in", "poly_max_mismatch", "min_quality", "min_length", "max_dust"):
            raise KeyError(k)
        if k == "poly_base" and isinstance(v, (str, bytes)):
            v = ord(v)
        setattr(p, k, int(v))
    _check(lib().mapad_clean_params_check(C.byref(p)), "mapad_clean_params_check")
    return p


def _clean_counts_dict(c):
    return {"reads_seen": int(c.reads_seen), "class_counts": np.array(c.class_counts[:], np.uint64), "bases_in": int(c.bases_in), "bases_out": int(c.bases_out),
            "bases_poly": int(c.bases_poly), "bases_trim5": int(c.bases_trim5), "bases_trim3": int(c.bases_trim3),
            "length_histogram": np.array(c.length_histogram[:], np.uint64), "dust_histogram": np.array(c.dust_histogram[:], np.uint64), "calls": int(c.calls)}


def _clean_result_dict(out):
    """copies a mapad_clean_result_t into numpy arrays and frees it"""
    r = out.contents
    n, total = int(r.n_reads), int(r.total_bases)

    def arr(p, count, dtype):
        return np.frombuffer(C.string_at(p, count * np.dtype(dtype).itemsize), dtype).copy() if count else np.zeros(0, dtype)
    d = {"n_reads": n, "cls": arr(r.cls, n, np.uint8), "trim5": arr(r.trim5, n, np.uint16), "trim3": arr(r.trim3, n, np.uint16), "poly_len": arr(r.poly_len, n, np.uint16),
         "dust": arr(r.dust, n, np.uint16), "seqs": arr(r.seqs, total, np.uint8), "quals": arr(r.quals, total, np.uint8), "offsets": arr(r.offsets, n + 1, np.uint64),
         "counts": _clean_counts_dict(r.counts), "kernel_ms": (float(r.kernel_ms[0]), float(r.kernel_ms[1]))}
    lib().mapad_clean_result_free(out)
    return d


def clean_reads_host(params, seqs, quals, offsets):
    """the clean-up rule on host threads, no GPU"""
    s, q, o = _packed(seqs, quals, offsets)
    out = C.POINTER(CleanResultC)()
    _check(lib().mapad_clean_reads_host(C.byref(params), _ptr(s), _ptr(q), _ptr(o), o.size - 1, C.byref(out)), "mapad_clean_reads_host")
    return _clean_result_dict(out)


class Cleaner:
    """mapad_cleaner_t: the clean-up stage on one device.  It needs no index and no Context."""

    def __init__(self, params, device_id=0):
        self.h = C.c_void_p()
        self.params = params
        _check(lib().mapad_cleaner_create(int(device_id), C.byref(params), C.byref(self.h)), "mapad_cleaner_create")

    def set_stream(self, stream_ptr):
        _check(lib().mapad_cleaner_set_stream(self.h, C.c_void_p(stream_ptr)), "mapad_cleaner_set_stream")

    def clean_reads(self, seqs, quals, offsets):
        s, q, o = _packed(seqs, quals, offsets)
        out = C.POINTER(CleanResultC)()
        _check(lib().mapad_clean_reads(self.h, _ptr(s), _ptr(q), _ptr(o), o.size - 1, C.byref(out)), "mapad_clean_reads")
        return _clean_result_dict(out)

    def clean_reads_device(self, d_seqs, d_quals, d_offsets, n_reads):
        """device pointers in, (d_seqs, d_quals, d_offsets, total_bases) out: the cleaner's own buffers, valid until its next call"""
        p = [C.c_void_p() for _ in range(3)]
        total = _u64()
        _check(lib().mapad_clean_reads_device(self.h, d_seqs, d_quals, d_offsets, int(n_reads), C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(total)),
               "mapad_clean_reads_device")
        return p[0].value, p[1].value, p[2].value, int(total.value)

    def totals(self):
        c = CleanCountsC()
        _check(lib().mapad_cleaner_totals(self.h, C.byref(c)), "mapad_cleaner_totals")
        return _clean_counts_dict(c)

    def reset(self):
        _check(lib().mapad_cleaner_reset(self.h), "mapad_cleaner_reset")

    def close(self):
        if self.h:
            lib().mapad_cleaner_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
