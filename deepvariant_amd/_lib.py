"""ctypes binding of libdvhip.so (the C ABI in include/dvhip.h).

The library is built in-tree by `deepvariant_amd/csrc/Makefile` (hipcc,
--offload-arch=gfx950) -- see `__graft_entry__.build()`.  There is no CPU
fallback: if the shared object is missing, loading raises, and every compute
entry point returns DV_ERR_NO_DEVICE without a GPU.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# DV_LIB_PATH: A/B runs of two builds (tools/); the product always loads the in-tree library
LIB_PATH = os.environ.get('DV_LIB_PATH') or os.path.join(_HERE, 'libdvhip.so')

DV_MAX_CHANNELS = 16
DV_READ_AUX_STRIDE = 8
DV_MEM_HOST, DV_MEM_DEVICE = 0, 1
DV_HP_NONE = -(1 << 31)

DV_OK = 0
DV_ERR_INVALID_ARGUMENT = -1
DV_ERR_UNSUPPORTED = -2
DV_ERR_NO_DEVICE = -3
DV_ERR_HIP = -4
DV_ERR_OUT_OF_MEMORY = -5
DV_ERR_BAD_INPUT = -6

# Every symbol include/dvhip.h declares (checked by tests/test_abi.py).
ABI_SYMBOLS = [
    'dv_last_error', 'dv_abi_version', 'dv_device_count',
    'dv_encoder_create', 'dv_encoder_destroy', 'dv_encode_batch', 'dv_base_aux_plane', 'dv_flow_channel_pixels',
    'dv_downsample_with_partition_mins',
    'dv_downsample_indices', 'dv_validate_batch', 'dv_query_reads', 'dv_crc32c',
    'dv_model_create', 'dv_model_destroy', 'dv_model_num_params', 'dv_model_conv_macs',
    'dv_model_num_layers', 'dv_model_layer_info', 'dv_model_load_weights', 'dv_model_calibrate', 'dv_model_apply_corrections',
    'dv_model_num_ops', 'dv_model_op_label', 'dv_model_probe_rounding', 'dv_model_set_blank_skip', 'dv_model_blank_thresholds', 'dv_model_is_precise',
    'dv_model_infer', 'dv_model_infer_rows', 'dv_model_output_info', 'dv_model_infer_outputs', 'dv_model_graph_stats', 'dv_model_debug_tensor', 'dv_set_profiling', 'dv_profile_ms',
    'dv_last_profile_count',
    'dv_bam_read_region', 'dv_read_table_fill_batch', 'dv_read_table_name',
    'dv_read_table_names', 'dv_read_table_ends', 'dv_read_table_free',
    'dv_cram_read_region', 'dv_cram_header', 'dv_read_table_aux_planes',
    'dv_pack_region', 'dv_packed_region_fill_batch', 'dv_packed_region_items',
    'dv_packed_region_free',
    'dv_pack_regions_device', 'dv_packed_regions_fill_batch', 'dv_packed_regions_download', 'dv_packed_regions_items',
    'dv_packed_regions_free', 'dv_pack_regions_device_last_stats',
    'dv_pack_draws_device', 'dv_pack_draws_device_last_stats',
    'dv_aligner_create', 'dv_aligner_destroy', 'dv_aligner_set_reference',
    'dv_aligner_set_haplotypes', 'dv_aligner_set_reads', 'dv_aligner_align_reads',
    'dv_aligner_stage', 'dv_aligner_fast_align', 'dv_aligner_haplotype_info',
    'dv_aligner_read_alignment', 'dv_aligner_merge_alignment', 'dv_aligner_is_normalized',
    'dv_aligner_score_threshold', 'dv_aligner_kmer_occurrences', 'dv_positions_map',
    'dv_merge_cigar_op', 'dv_local_align', 'dv_local_align_many',
    'dv_local_align_pairs_device', 'dv_local_align_device_last_stats', 'dv_realign_regions_device',
    'dv_local_align_device_last_traceback_stats', 'dv_local_align_band',
    'dv_fast_pass_batch', 'dv_fast_pass_batch_device', 'dv_fast_pass_device_last_stats',
    'dv_trim_reads_batch', 'dv_trim_reads_batch_device', 'dv_trimmed_reads_arrays', 'dv_trimmed_reads_free',
    'dv_trim_device_last_stats',
    'dv_alt_align_batch', 'dv_alt_align_batch_device', 'dv_alt_aligned_arrays', 'dv_alt_aligned_free',
    'dv_alt_align_device_last_stats',
    'dv_align_windows_batch', 'dv_align_windows_batch_device', 'dv_aligned_windows_arrays', 'dv_aligned_windows_free',
    'dv_realign_finish_last_stats', 'dv_realign_finish_sorted_order',
    'dv_debruijn_build', 'dv_debruijn_destroy', 'dv_debruijn_kmer_size', 'dv_debruijn_haplotypes',
    'dv_debruijn_graphviz', 'dv_debruijn_compact_batch', 'dv_debruijn_compact_batch_device', 'dv_debruijn_compact_free',
    'dv_debruijn_paths_batch', 'dv_debruijn_paths_batch_device', 'dv_debruijn_paths_free', 'dv_debruijn_paths_last_stats',
    'dv_debruijn_device_last_stats', 'dv_debruijn_from_compact', 'dv_realign_regions', 'dv_realign_result_free', 'dv_phase_reads',
    'dv_phase_reads_batch', 'dv_phase_reads_batch_device', 'dv_phase_device_last_stats',
    'dv_count_alleles', 'dv_count_alleles_batch', 'dv_allele_counts_arrays', 'dv_allele_counts_free', 'dv_merge_alt_channels',
    'dv_count_alleles_gvcf_batch', 'dv_gvcf_blocks_arrays', 'dv_gvcf_blocks_free',
    'dv_call_candidates_batch', 'dv_candidates_arrays', 'dv_candidates_free',
    'dv_select_windows_batch', 'dv_windows_arrays', 'dv_windows_free', 'dv_count_batch_last_stats',
    'dv_genotype_sites', 'dv_genotype_sites_device', 'dv_genotypes_arrays', 'dv_genotypes_free',
    'dv_genotype_min_nonref_prob', 'dv_genotype_device_last_stats',
    'dv_gvcf_merge', 'dv_gvcf_merge_device', 'dv_gvcf_merged_arrays', 'dv_gvcf_merged_free',
    'dv_gvcf_merge_scan_chunk', 'dv_gvcf_merge_last_stats',
    'dv_gvcf_rows', 'dv_gvcf_rows_device', 'dv_gvcf_text_arrays', 'dv_gvcf_text_free', 'dv_gvcf_rows_last_stats',
    'dv_bgzf_params', 'dv_bgzf_compress', 'dv_bgzf_compress_device', 'dv_bgzf_arrays', 'dv_bgzf_free', 'dv_bgzf_last_stats',
    'dv_gvcf_rows_bgzf', 'dv_gvcf_rows_bgzf_device',
]

DV_GENOTYPE_DEVICE_MAX_ALTS = 6
DV_GENOTYPE_OK, DV_GENOTYPE_BAD_SUM, DV_GENOTYPE_INCOMPLETE = 0, 1, 2


# dv_ref_fetch_fn (include/dvhip.h): the reference bases a CRAM written against an external FASTA leaves out
REF_FETCH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_char_p, C.c_int64, C.c_int64, C.POINTER(C.c_char),
                           C.POINTER(C.c_int64))


class DvError(RuntimeError):
  """A non-zero dv_status; `.status` carries the code."""

  def __init__(self, status, message):
    super().__init__('libdvhip status %d: %s' % (status, message))
    self.status = status


class DvEncoderOptions(C.Structure):
  _fields_ = [
      ('width', C.c_int32), ('height', C.c_int32),
      ('reference_band_height', C.c_int32), ('n_channels', C.c_int32),
      ('channels', C.c_int32 * DV_MAX_CHANNELS),
      ('base_color_offset_a_and_g', C.c_int32),
      ('base_color_offset_t_and_c', C.c_int32),
      ('base_color_stride', C.c_int32),
      ('allele_supporting_read_alpha', C.c_float),
      ('allele_unsupporting_read_alpha', C.c_float),
      ('other_allele_supporting_read_alpha', C.c_float),
      ('reference_matching_read_alpha', C.c_float),
      ('reference_mismatching_read_alpha', C.c_float),
      ('indel_anchoring_base_char', C.c_int32),
      ('reference_base_quality', C.c_int32),
      ('positive_strand_color', C.c_int32),
      ('negative_strand_color', C.c_int32),
      ('base_quality_cap', C.c_int32), ('mapping_quality_cap', C.c_int32),
      ('min_base_quality', C.c_int32), ('min_mapping_quality', C.c_int32),
      ('random_seed', C.c_uint32),
      ('sort_by_haplotypes', C.c_int32),
      ('hp_tag_for_assembly_polishing', C.c_int32),
      ('sort_by_alt_allele_support', C.c_int32),
      ('min_non_zero_allele_frequency', C.c_float),
  ]


class DvBatch(C.Structure):
  _fields_ = [
      ('memory', C.c_int32),
      ('n_reads', C.c_int32),
      ('read_pos', C.c_void_p), ('read_sort_pos', C.c_void_p),
      ('read_seq_off', C.c_void_p), ('read_cigar_off', C.c_void_p),
      ('read_mapq', C.c_void_p), ('read_flags', C.c_void_p),
      ('read_frag_len', C.c_void_p), ('read_hp', C.c_void_p),
      ('read_name_rank', C.c_void_p), ('read_aux', C.c_void_p),
      ('bases', C.c_void_p), ('quals', C.c_void_p),
      ('mod_5mc', C.c_void_p), ('mod_6ma', C.c_void_p),
      ('cigar', C.c_void_p),
      ('n_bases', C.c_uint32), ('n_cigar', C.c_uint32),
      ('n_items', C.c_int32),
      ('item_variant_start', C.c_void_p), ('item_image_start', C.c_void_p),
      ('item_ref_idx', C.c_void_p), ('item_list_off', C.c_void_p),
      ('item_height', C.c_void_p), ('item_out_off', C.c_void_p),
      ('item_blank_mask', C.c_void_p), ('item_mean_coverage', C.c_void_p),
      ('ref_windows', C.c_void_p), ('n_ref_windows', C.c_uint32),
      ('list_read', C.c_void_p), ('list_code', C.c_void_p),
      ('list_group', C.c_void_p), ('list_aux', C.c_void_p),
      ('n_list', C.c_uint32), ('max_list_len', C.c_uint32),
      ('base_aux0', C.c_void_p), ('base_aux1', C.c_void_p),
      ('ref_aux0', C.c_void_p), ('ref_aux1', C.c_void_p), ('ref_aux2', C.c_void_p),
      ('base_aux2', C.c_void_p),        # ABI v6
      ('max_cigar_ops', C.c_uint32), ('max_item_height', C.c_uint32),   # ABI v7: LDS sizing hints, 0 = unknown
  ]


class DvReadRequirements(C.Structure):
  _fields_ = [('keep_duplicates', C.c_int32),
              ('keep_failed_vendor_quality_checks', C.c_int32),
              ('keep_secondary_alignments', C.c_int32),
              ('keep_supplementary_alignments', C.c_int32),
              ('keep_improperly_placed', C.c_int32),
              ('min_mapping_quality', C.c_int32),
              ('use_original_base_quality_scores', C.c_int32),
              ('parse_base_modifications', C.c_int32),      # ABI v6: MM / ML / MN -> 5mC / 6mA planes
              ('parse_flow_tags', C.c_int32)]               # ABI v6: tp / t0 planes


class DvPackReads(C.Structure):
  _fields_ = [('n_reads', C.c_int32), ('read_pos', C.c_void_p), ('read_end', C.c_void_p),
              ('names', C.c_void_p), ('name_off', C.c_void_p), ('read_number', C.c_void_p)]


class DvPackOptions(C.Structure):
  _fields_ = [('width', C.c_int32), ('read_overlap_buffer_bp', C.c_int32),
              ('pileup_height', C.c_int32), ('n_threads', C.c_int32), ('example_bytes', C.c_uint64)]


class DvPackCandidate(C.Structure):
  _fields_ = [('start', C.c_int64), ('end', C.c_int64), ('n_alts', C.c_int32),
              ('ref_idx', C.c_int32), ('first_combo', C.c_uint32), ('n_combos', C.c_uint32),
              ('first_support', C.c_uint32), ('n_support', C.c_uint32)]


class DvAlignerOptions(C.Structure):
  _fields_ = [('match', C.c_int32), ('mismatch', C.c_int32), ('gap_open', C.c_int32),
              ('gap_extend', C.c_int32), ('kmer_size', C.c_int32), ('read_size', C.c_int32),
              ('max_num_of_mismatches', C.c_int32),
              ('realignment_similarity_threshold', C.c_double),
              ('force_alignment', C.c_int32), ('normalize_reads', C.c_int32),
              ('ref_prefix_len', C.c_int32), ('ref_suffix_len', C.c_int32)]


class DvRealignedRead(C.Structure):
  _fields_ = [('status', C.c_int32), ('n_cigar', C.c_int32), ('position', C.c_int64),
              ('cigar_off', C.c_uint32), ('reserved', C.c_uint32)]


class DvReadAlignment(C.Structure):
  _fields_ = [('position', C.c_int32), ('score', C.c_int32), ('cigar', C.c_char * 120)]


class DvLocalAlignment(C.Structure):
  _fields_ = [('score', C.c_int32), ('ref_begin', C.c_int32), ('ref_end', C.c_int32),
              ('query_begin', C.c_int32), ('query_end', C.c_int32), ('mismatches', C.c_int32),
              ('cigar', C.c_char * 512)]


# include/dvhip.h: what one pair may measure for the device form of the local aligner (longer ones are
# aligned by the host code inside the same call)
DV_LOCAL_ALIGN_DEVICE_MAX_QUERY = 2048
DV_LOCAL_ALIGN_DEVICE_MAX_REFERENCE = 65534


class DvRealignDeviceStats(C.Structure):
  _fields_ = [('pairs', C.c_int64), ('pairs_on_host', C.c_int64), ('cells', C.c_int64), ('launches', C.c_int64)]


# include/dvhip.h: what the device's banded trace-back holds per pair (one band diagonal per lane; run words);
# a pair past either is traced back by the host code inside the same call
DV_LOCAL_ALIGN_DEVICE_MAX_BAND = 31
DV_LOCAL_ALIGN_DEVICE_MAX_RUNS = 64


# include/dvhip.h: what one haplotype may measure for the device form of the fast pass (it lives in LDS; a longer one
# is run by the host code inside the same call), and the largest match / mismatch value the kernel takes
DV_FAST_PASS_DEVICE_MAX_HAPLOTYPE = 8192
DV_FAST_PASS_DEVICE_MAX_SCORING = 32767


class DvFastPassWindow(C.Structure):
  _fields_ = [('first_read', C.c_int32), ('n_reads', C.c_int32), ('first_haplotype', C.c_int32),
              ('n_haplotypes', C.c_int32), ('reference', C.c_int32), ('ref_prefix_len', C.c_int32),
              ('ref_suffix_len', C.c_int32), ('reserved', C.c_int32)]


class DvFastPassStats(C.Structure):
  _fields_ = [('haplotypes', C.c_int64), ('haplotypes_on_host', C.c_int64), ('pairs', C.c_int64),
              ('cells', C.c_int64), ('launches', C.c_int64)]


class DvTrimWindow(C.Structure):
  _fields_ = [('q0', C.c_int64), ('q1', C.c_int64), ('r0', C.c_int64), ('r1', C.c_int64),
              ('min_overlap', C.c_int32), ('reserved', C.c_int32)]


class DvTrimmedReadsView(C.Structure):
  _fields_ = [('n_windows', C.c_int32), ('n_rows', C.c_int32), ('n_words', C.c_int64),
              ('window_row_off', C.c_void_p), ('src_row', C.c_void_p), ('pos', C.c_void_p), ('end', C.c_void_p),
              ('read_trim', C.c_void_p), ('new_len', C.c_void_p), ('cigar_off', C.c_void_p), ('cigar', C.c_void_p)]


class DvPackRows(C.Structure):
  _fields_ = [('n_reads', C.c_int32), ('read_pos', C.c_void_p), ('read_end', C.c_void_p), ('read_key', C.c_void_p)]


class DvPackRegionSlice(C.Structure):
  _fields_ = [('read_first', C.c_int32), ('n_reads', C.c_int32), ('cand_first', C.c_int32), ('n_cands', C.c_int32)]


class DvPackRegionsOptions(C.Structure):
  _fields_ = [('width', C.c_int32), ('read_overlap_buffer_bp', C.c_int32), ('pileup_height', C.c_int32),
              ('n_candidates', C.c_int32), ('n_combo_masks', C.c_uint32), ('n_support', C.c_uint32),
              ('example_bytes', C.c_uint64), ('mean_coverage', C.c_float)]


class DvPackedRegionsView(C.Structure):
  _fields_ = [('n_items', C.c_int32), ('n_list', C.c_uint32), ('max_list_len', C.c_uint32)] + [
      (name, C.c_void_p) for name in (
          'item_variant_start', 'item_image_start', 'item_ref_idx', 'item_list_off', 'item_height', 'item_out_off',
          'item_mean_coverage', 'item_candidate', 'item_combo', 'list_read', 'list_code', 'list_group')]


class DvPackDeviceStats(C.Structure):
  _fields_ = [('regions', C.c_int64), ('candidates', C.c_int64), ('items', C.c_int64), ('list_entries', C.c_int64),
              ('regions_unsorted', C.c_int64), ('launches', C.c_int64)]


class DvPackDraw(C.Structure):
  _fields_ = [('cand', C.c_int32), ('combo_mask', C.c_uint32), ('row_first', C.c_int32), ('n_rows', C.c_int32),
              ('ref_idx', C.c_uint32), ('variant_start', C.c_int32), ('image_start', C.c_int32), ('height', C.c_uint16),
              ('out_off', C.c_uint64), ('mean_coverage', C.c_float)]


class DvPackDrawsStats(C.Structure):
  _fields_ = [('draws', C.c_int64), ('candidates', C.c_int64), ('list_entries', C.c_int64), ('launches', C.c_int64)]


class DvTrimStats(C.Structure):
  _fields_ = [('pairs_tested', C.c_int64), ('pairs_kept', C.c_int64), ('words_read', C.c_int64),
              ('words_written', C.c_int64), ('launches', C.c_int64)]


class DvAltAlignItem(C.Structure):
  _fields_ = [('first_row', C.c_int32), ('n_rows', C.c_int32), ('target', C.c_int32), ('read_size', C.c_int32),
              ('ref_start', C.c_int64), ('reserved', C.c_int64)]


class DvAltAlignedView(C.Structure):
  _fields_ = [('n_items', C.c_int32), ('n_pairs', C.c_int32), ('n_words', C.c_int64),
              ('item_pair_off', C.c_void_p), ('status', C.c_void_p), ('position', C.c_void_p),
              ('cigar_off', C.c_void_p), ('cigar', C.c_void_p)]


class DvAltAlignStats(C.Structure):
  _fields_ = [(n, C.c_int64) for n in ('items', 'items_on_host', 'pairs', 'pairs_fast', 'pairs_swept',
                                       'pairs_swept_on_host', 'pairs_traced_on_host', 'status0', 'status1', 'status2',
                                       'words_written', 'launches')]


class DvAlignWindow(C.Structure):
  _fields_ = [('first_read', C.c_int32), ('n_reads', C.c_int32), ('first_haplotype', C.c_int32),
              ('n_haplotypes', C.c_int32), ('reference', C.c_int32), ('ref_prefix_len', C.c_int32),
              ('ref_suffix_len', C.c_int32), ('reserved', C.c_int32), ('ref_start', C.c_int64)]


class DvAlignedWindowsView(C.Structure):
  _fields_ = [('n_windows', C.c_int32), ('n_reads', C.c_int32), ('n_words', C.c_int64),
              ('window_read_off', C.c_void_p), ('status', C.c_void_p), ('position', C.c_void_p),
              ('cigar_off', C.c_void_p), ('cigar', C.c_void_p)]


class DvRealignFinishStats(C.Structure):
  _fields_ = [(n, C.c_int64) for n in ('windows', 'windows_on_host', 'reads', 'cigar_words', 'launches', 'bytes_down')]


class DvGenotypesView(C.Structure):
  _fields_ = [('n_sites', C.c_int32), ('reserved', C.c_int32), ('n_items', C.c_int64), ('n_predictions', C.c_int64),
              ('rounded', C.c_void_p), ('pred_off', C.c_void_p), ('predictions', C.c_void_p), ('best', C.c_void_p),
              ('removed', C.c_void_p), ('status', C.c_void_p)]


class DvGenotypeDeviceStats(C.Structure):
  _fields_ = [(n, C.c_int64) for n in ('sites', 'sites_on_host', 'launches', 'bytes_down')]


class DvGvcfMergedView(C.Structure):
  _fields_ = [('n_pieces', C.c_int64), ('n_variants', C.c_int64), ('piece_start', C.c_void_p), ('piece_end', C.c_void_p),
              ('piece_block', C.c_void_p), ('piece_slot', C.c_void_p), ('var_slot', C.c_void_p)]


class DvGvcfMergeStats(C.Structure):
  _fields_ = [(n, C.c_int64) for n in ('blocks', 'variants', 'pieces', 'launches', 'bytes_up', 'bytes_down')]


class DvGvcfRowsInput(C.Structure):
  _fields_ = [('n_groups', C.c_int32), ('med_dp', C.c_int32), ('want_row_off', C.c_int32), ('reserved', C.c_int32),
              ('block_off', C.c_void_p), ('var_off', C.c_void_p), ('blocks', C.c_void_p), ('var_start', C.c_void_p),
              ('var_end', C.c_void_p), ('var_end_base', C.c_void_p), ('var_text_off', C.c_void_p),
              ('var_text', C.c_void_p), ('name_off', C.c_void_p), ('names', C.c_void_p)]


class DvGvcfTextView(C.Structure):
  _fields_ = [('text', C.c_void_p), ('n_bytes', C.c_int64), ('row_off', C.c_void_p), ('n_rows', C.c_int64),
              ('n_pieces', C.c_int64), ('med_dp', C.c_int32), ('reserved', C.c_int32)]


class DvGvcfRowsStats(C.Structure):
  _fields_ = [(n, C.c_int64) for n in ('blocks', 'variants', 'pieces', 'rows', 'text_bytes', 'launches', 'bytes_up',
                                       'bytes_down')]


class DvBgzfParameters(C.Structure):
  _fields_ = [(n, C.c_int32) for n in ('block', 'tile', 'seg', 'hash_bits')]


class DvBgzfView(C.Structure):
  _fields_ = [('data', C.c_void_p), ('n_bytes', C.c_int64), ('n_blocks', C.c_int64), ('block_coff', C.c_void_p),
              ('stored_blocks', C.c_int64)]


class DvBgzfStats(C.Structure):
  _fields_ = [(n, C.c_int64) for n in ('text_bytes', 'file_bytes', 'blocks', 'stored_blocks', 'launches', 'bytes_up',
                                       'bytes_down')]


class DvGvcfRowsMeta(C.Structure):
  _fields_ = [('n_rows', C.c_int64), ('n_pieces', C.c_int64), ('text_bytes', C.c_int64), ('row_off', C.c_void_p)]


class DvRealignTracebackStats(C.Structure):
  _fields_ = [('traced_on_device', C.c_int64), ('traced_on_host', C.c_int64), ('band_cells', C.c_int64),
              ('widest_band', C.c_int64)]


class DvDebruijnOptions(C.Structure):
  _fields_ = [(n, C.c_int32) for n in ('min_k', 'max_k', 'step_k', 'min_mapq', 'min_base_quality',
                                       'min_edge_weight', 'max_num_paths', 'disable_graph_pruning')]


# include/dvhip.h: what one window may measure for the device form of the assembly (a larger one is built by the host
# code inside the same call)
DV_DEBRUIJN_DEVICE_MAX_VERTICES = 8192
DV_DEBRUIJN_DEVICE_MAX_EDGES = 8192
DV_DEBRUIJN_DEVICE_MAX_BASES = 131072


class DvDebruijnWindow(C.Structure):
  _fields_ = [('reference', C.c_int32), ('first_read', C.c_int32), ('n_reads', C.c_int32), ('reserved', C.c_int32)]


class DvDebruijnCompact(C.Structure):
  _fields_ = [('k', C.POINTER(C.c_int32)), ('k_tries', C.POINTER(C.c_int32)), ('vertex_off', C.POINTER(C.c_int64)),
              ('vertex_seq', C.POINTER(C.c_int32)), ('vertex_pos', C.POINTER(C.c_int32)),
              ('edge_off', C.POINTER(C.c_int64)), ('edge_from', C.POINTER(C.c_int32)), ('edge_to', C.POINTER(C.c_int32)),
              ('edge_weight', C.POINTER(C.c_int32)), ('edge_is_ref', C.POINTER(C.c_int32)),
              ('edge_seq', C.POINTER(C.c_int32)), ('edge_pos', C.POINTER(C.c_int32))]


class DvDebruijnDeviceStats(C.Structure):
  _fields_ = [('windows', C.c_int64), ('windows_on_host', C.c_int64), ('kmers', C.c_int64), ('k_tries', C.c_int64),
              ('launches', C.c_int64), ('windows_rejected', C.c_int64)]


# include/dvhip.h: what the device form of pruning and path enumeration covers (a call with a larger max_num_paths, and
# a window whose haplotypes' text is longer, are computed by the host code inside the same call)
DV_DEBRUIJN_DEVICE_MAX_PATHS = 1024
DV_DEBRUIJN_DEVICE_MAX_HAP_BYTES = 262144
DV_DEBRUIJN_PATHS_OK, DV_DEBRUIJN_PATHS_NO_GRAPH, DV_DEBRUIJN_PATHS_TOO_MANY = 0, 1, 2


class DvDebruijnPaths(C.Structure):
  _fields_ = [('k', C.POINTER(C.c_int32)), ('status', C.POINTER(C.c_int32)), ('hap_first', C.POINTER(C.c_int32)),
              ('hap_off', C.POINTER(C.c_int64)), ('hap_text', C.POINTER(C.c_char))]


class DvDebruijnPathsStats(C.Structure):
  _fields_ = [('windows', C.c_int64), ('windows_on_host', C.c_int64), ('paths', C.c_int64), ('hap_bytes', C.c_int64),
              ('launches', C.c_int64), ('bytes_down', C.c_int64)]


class DvRealignRegion(C.Structure):
  _fields_ = [('bases', C.c_void_p), ('quals', C.c_void_p), ('n_bases', C.c_int64), ('read_seq_off', C.c_void_p),
              ('read_mapq', C.c_void_p), ('read_start', C.c_void_p), ('read_end', C.c_void_p),
              ('n_reads', C.c_int32), ('n_windows', C.c_int32), ('window_start', C.c_void_p),
              ('window_end', C.c_void_p), ('ref', C.c_char_p), ('ref_start', C.c_int64), ('ref_len', C.c_int64),
              ('contig_len', C.c_int64)]


class DvRealignOptions(C.Structure):
  _fields_ = [('dbg', DvDebruijnOptions), ('aln', DvAlignerOptions), ('ref_align_margin', C.c_int32),
              ('n_threads', C.c_int32)]


class DvRealignOutput(C.Structure):
  _fields_ = [('region_row_off', C.POINTER(C.c_int64)), ('order', C.POINTER(C.c_int32)),
              ('status', C.POINTER(C.c_int32)), ('position', C.POINTER(C.c_int64)),
              ('cigar_off', C.POINTER(C.c_int64)), ('cigar', C.POINTER(C.c_uint32)),
              ('region_assembled_off', C.POINTER(C.c_int32)), ('assembled_window', C.POINTER(C.c_int32)),
              ('assembled_hap_off', C.POINTER(C.c_int32)), ('hap_text_off', C.POINTER(C.c_int64)),
              ('hap_text', C.POINTER(C.c_char))]


class DvPhasingAllele(C.Structure):
  _fields_ = [('bases_off', C.c_int64), ('bases_len', C.c_int32), ('is_ref', C.c_int32),
              ('support_off', C.c_int64), ('n_support', C.c_int32), ('reserved', C.c_int32)]


class DvPhasingCandidate(C.Structure):
  _fields_ = [('start', C.c_int64), ('end', C.c_int64), ('allele_off', C.c_int32), ('n_alleles', C.c_int32)]


class DvPhasingRegion(C.Structure):
  _fields_ = [('candidate_off', C.c_int32), ('n_candidates', C.c_int32), ('allele_off', C.c_int32),
              ('n_alleles', C.c_int32), ('support_off', C.c_int64), ('n_support', C.c_int64),
              ('first_read', C.c_int64), ('n_reads', C.c_int32), ('reserved', C.c_int32)]


class DvPhasingStats(C.Structure):
  _fields_ = [('regions', C.c_int64), ('regions_on_host', C.c_int64), ('sites_in_graphs', C.c_int64),
              ('vertices', C.c_int64), ('combinations', C.c_int64), ('launches', C.c_int64)]


DV_PHASING_DEVICE_MAX_READS = 1024
DV_PHASING_DEVICE_MAX_VERTICES = 8


class DvAltMergeEntry(C.Structure):
  _fields_ = [('example', C.c_int64), ('first_row', C.c_int32), ('rows', C.c_int32),
              ('scratch_alt1', C.c_int64), ('scratch_alt2', C.c_int64)]


class DvAlleleCounterOptions(C.Structure):
  _fields_ = [('interval_start', C.c_int64), ('interval_end', C.c_int64),
              ('reads_interval_start', C.c_int64), ('reads_interval_end', C.c_int64),
              ('ref_bases', C.c_char_p), ('ref_start', C.c_int64), ('n_ref_bases', C.c_int64),
              ('contig_n_bases', C.c_int64), ('min_mapping_quality', C.c_int32),
              ('min_base_quality', C.c_int32), ('keep_legacy_behavior', C.c_int32),
              ('track_ref_reads', C.c_int32), ('candidate_positions', C.c_void_p),
              ('n_candidate_positions', C.c_int32)]


class DvAlleleEvent(C.Structure):
  # include/dvhip.h dv_allele_event (ABI v3): length_type = length (bits 0-27) | AlleleType (28-30) |
  # is_low_quality (bit 31)
  _fields_ = [('position', C.c_int32), ('read', C.c_uint32), ('read_offset', C.c_uint32),
              ('length_type', C.c_uint32)]


class DvGvcfSite(C.Structure):
  # include/dvhip.h dv_gvcf_site: one entry of the reference-confidence table
  _fields_ = [('likelihoods', C.c_double * 3), ('gq', C.c_int32), ('has_valid_gl', C.c_int32)]


class DvGvcfOptions(C.Structure):
  _fields_ = [('p_error', C.c_double), ('max_gq', C.c_int32), ('gq_resolution', C.c_int32),
              ('max_cache_coverage', C.c_int32), ('include_med_dp', C.c_int32),
              ('left_padding', C.c_int32), ('right_padding', C.c_int32),
              ('table', C.c_void_p), ('n_table', C.c_int64)]


class DvGvcfBlock(C.Structure):
  _fields_ = [('start', C.c_int64), ('end', C.c_int64), ('likelihoods', C.c_double * 3),
              ('gq', C.c_int32), ('min_dp', C.c_int32), ('med_dp', C.c_int32),
              ('ref_base', C.c_uint8), ('has_valid_gl', C.c_uint8), ('reserved', C.c_uint8 * 2)]


class DvCandidateOptions(C.Structure):
  # include/dvhip.h dv_candidate_options: the thresholds are C floats (the reference's proto `float` fields)
  _fields_ = [('min_count_snps', C.c_int32), ('min_count_indels', C.c_int32),
              ('min_fraction_snps', C.c_float), ('min_fraction_indels', C.c_float),
              ('track_ref_reads', C.c_int32), ('positions_only', C.c_int32)]


class DvWindowOptions(C.Structure):
  # include/dvhip.h dv_window_options: the coefficients are C floats, the boundary a double (as the reference compares)
  _fields_ = [('model_type', C.c_int32), ('min_num_supporting_reads', C.c_int32), ('max_num_supporting_reads', C.c_int32),
              ('min_allele_support', C.c_int32), ('enable_strict_insertion_filter', C.c_int32),
              ('bias', C.c_float), ('coeff_soft_clip', C.c_float), ('coeff_substitution', C.c_float),
              ('coeff_insertion', C.c_float), ('coeff_deletion', C.c_float), ('coeff_reference', C.c_float),
              ('min_windows_distance', C.c_int32), ('decision_boundary', C.c_double),
              ('want_debug', C.c_int32), ('reserved', C.c_int32)]


class DvCountBatchStats(C.Structure):
  # include/dvhip.h dv_count_batch_stats
  _fields_ = [('regions', C.c_int32), ('regions_batched', C.c_int32), ('regions_alone', C.c_int32),
              ('count_launches', C.c_int32), ('count_workgroups', C.c_int64)]


class DvCandidateSite(C.Structure):
  _fields_ = [('offset', C.c_int32), ('ref_count', C.c_int32), ('total', C.c_int32),
              ('first_allele', C.c_int32), ('n_alleles', C.c_int32)]


class DvCandidateAllele(C.Structure):
  _fields_ = [('length_type', C.c_uint32), ('count', C.c_int32), ('read', C.c_uint32), ('read_offset', C.c_uint32)]


class DvModelDesc(C.Structure):
  _fields_ = [('height', C.c_int32), ('width', C.c_int32),
              ('channels', C.c_int32), ('num_classes', C.c_int32),
              ('max_batch', C.c_int32)]


_lib = None


def build(force: bool = False) -> str:
  """Compiles libdvhip.so for gfx950 with the committed Makefile."""
  args = ['make', '-C', os.path.join(_HERE, 'csrc')]
  if force:
    subprocess.check_call(args + ['clean'], stdout=subprocess.DEVNULL)
  subprocess.check_call(args, stdout=subprocess.DEVNULL)
  return LIB_PATH


def lib():
  """Loads libdvhip.so; raises if it has not been built (no fallback)."""
  global _lib
  if _lib is None:
    if not os.path.exists(LIB_PATH):
      raise ImportError(
          'deepvariant_amd/libdvhip.so is missing: run '
          '`python -c "import __graft_entry__ as g; g.build()"` '
          '(there is no CPU fallback for the HIP hot path)')
    try:
      # PyTorch wheels bundle their own libamdhip64 / libhsa-runtime64.  If /opt/rocm's
      # copies (libdvhip.so's DT_NEEDED) get into the process first, torch later finds
      # "No HIP GPUs"; loaded after torch, libdvhip.so binds to torch's runtime by SONAME
      # and both share one device context.  Without torch this is a plain ROCm library.
      import torch  # noqa: F401  pylint: disable=unused-import,g-import-not-at-top
    except ImportError:
      pass
    l = C.CDLL(LIB_PATH)
    l.dv_last_error.restype = C.c_char_p
    l.dv_crc32c.restype = C.c_uint32
    l.dv_crc32c.argtypes = [C.c_void_p, C.c_size_t]
    l.dv_profile_ms.restype = C.c_double
    l.dv_model_num_params.restype = C.c_int64
    l.dv_model_num_params.argtypes = [C.c_void_p]
    l.dv_model_conv_macs.restype = C.c_int64
    l.dv_model_conv_macs.argtypes = [C.c_void_p]
    l.dv_model_num_layers.argtypes = [C.c_void_p]
    l.dv_model_destroy.argtypes = [C.c_void_p]
    l.dv_encoder_destroy.argtypes = [C.c_void_p]
    l.dv_validate_batch.argtypes = [C.c_void_p, C.c_int32]
    l.dv_encode_batch.argtypes = [
        C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
        C.c_void_p]
    l.dv_model_infer.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                 C.c_void_p]
    l.dv_model_load_weights.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    l.dv_model_calibrate.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    l.dv_model_apply_corrections.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    l.dv_model_num_ops.argtypes = [C.c_void_p]
    l.dv_model_infer_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    l.dv_model_set_blank_skip.argtypes = [C.c_void_p, C.c_int]
    l.dv_model_is_precise.argtypes = [C.c_void_p]
    l.dv_model_blank_thresholds.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    l.dv_model_op_label.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int]
    l.dv_model_probe_rounding.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    l.dv_model_graph_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    l.dv_model_output_info.argtypes = [C.c_void_p, C.c_char_p] + [C.c_void_p] * 3
    l.dv_model_infer_outputs.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
    l.dv_model_layer_info.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
    l.dv_bam_read_region.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.c_int64,
                                     C.c_void_p, C.c_int, C.c_void_p]
    l.dv_cram_read_region.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_void_p, REF_FETCH_FN,
                                      C.c_void_p, C.c_int, C.c_void_p]
    l.dv_cram_header.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p]
    l.dv_read_table_aux_planes.argtypes = [C.c_void_p] * 6
    l.dv_downsample_with_partition_mins.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                                    C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    l.dv_base_aux_plane.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    l.dv_flow_channel_pixels.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.c_void_p]
    l.dv_read_table_fill_batch.argtypes = [C.c_void_p, C.c_void_p]
    l.dv_read_table_name.restype = C.c_char_p
    l.dv_read_table_name.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    l.dv_read_table_names.argtypes = [C.c_void_p] + [C.c_void_p] * 4
    l.dv_pack_region.argtypes = [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 6
    l.dv_packed_region_fill_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    l.dv_packed_region_items.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    l.dv_packed_region_free.argtypes = [C.c_void_p]
    l.dv_pack_regions_device.argtypes = [C.c_int32] + [C.c_void_p] * 9
    l.dv_packed_regions_fill_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    l.dv_packed_regions_download.argtypes = [C.c_void_p, C.c_void_p]
    l.dv_packed_regions_items.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    l.dv_packed_regions_free.argtypes = [C.c_void_p]
    l.dv_packed_regions_free.restype = None
    l.dv_pack_regions_device_last_stats.argtypes = [C.c_void_p]
    l.dv_pack_draws_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    l.dv_pack_draws_device_last_stats.argtypes = [C.c_void_p]
    l.dv_read_table_ends.restype = C.c_void_p
    l.dv_read_table_ends.argtypes = [C.c_void_p]
    l.dv_read_table_free.argtypes = [C.c_void_p]
    l.dv_aligner_create.argtypes = [C.c_void_p, C.c_void_p]
    l.dv_aligner_destroy.argtypes = [C.c_void_p]
    l.dv_aligner_destroy.restype = None
    l.dv_aligner_set_reference.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    l.dv_aligner_set_haplotypes.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    l.dv_aligner_set_reads.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    l.dv_aligner_align_reads.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    l.dv_aligner_stage.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    l.dv_aligner_fast_align.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p]
    l.dv_aligner_haplotype_info.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 5 + [C.c_int32]
    l.dv_aligner_read_alignment.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    l.dv_aligner_merge_alignment.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_char_p, C.c_char_p,
                                             C.c_void_p, C.c_int32]
    l.dv_aligner_is_normalized.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_char_p]
    l.dv_aligner_score_threshold.argtypes = [C.c_void_p]
    l.dv_aligner_kmer_occurrences.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_void_p]
    l.dv_positions_map.argtypes = [C.c_char_p, C.c_int32, C.c_void_p]
    l.dv_merge_cigar_op.argtypes = [C.c_void_p, C.c_int32, C.c_char, C.c_int32, C.c_int32]
    l.dv_local_align.argtypes = [C.c_char_p, C.c_char_p] + [C.c_int32] * 4 + [C.c_void_p]
    l.dv_local_align_many.argtypes = [C.c_char_p, C.c_int32, C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p]
    l.dv_local_align_pairs_device.argtypes = ([C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p] +
                                              [C.c_int32] * 4 + [C.c_void_p, C.c_void_p])
    l.dv_local_align_device_last_stats.argtypes = [C.c_void_p]
    l.dv_local_align_device_last_traceback_stats.argtypes = [C.c_void_p]
    l.dv_local_align_band.argtypes = [C.c_char_p, C.c_char_p] + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p]
    for fn in (l.dv_fast_pass_batch, l.dv_fast_pass_batch_device):
      fn.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 7
    l.dv_fast_pass_device_last_stats.argtypes = [C.c_void_p]
    l.dv_trim_reads_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    l.dv_trim_reads_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    l.dv_trimmed_reads_arrays.argtypes = [C.c_void_p, C.c_void_p]
    l.dv_trimmed_reads_free.argtypes = [C.c_void_p]
    l.dv_trimmed_reads_free.restype = None
    l.dv_trim_device_last_stats.argtypes = [C.c_void_p]
    l.dv_alt_align_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]
    l.dv_alt_align_batch_device.argtypes = l.dv_alt_align_batch.argtypes + [C.c_void_p]
    l.dv_alt_aligned_arrays.argtypes = [C.c_void_p, C.c_void_p]
    l.dv_alt_aligned_free.argtypes = [C.c_void_p]
    l.dv_alt_aligned_free.restype = None
    l.dv_alt_align_device_last_stats.argtypes = [C.c_void_p]
    l.dv_align_windows_batch.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
    l.dv_align_windows_batch_device.argtypes = l.dv_align_windows_batch.argtypes + [C.c_void_p]
    l.dv_aligned_windows_arrays.argtypes = [C.c_void_p, C.c_void_p]
    l.dv_aligned_windows_free.argtypes = [C.c_void_p]
    l.dv_aligned_windows_free.restype = None
    l.dv_realign_finish_last_stats.argtypes = [C.c_void_p]
    l.dv_realign_finish_sorted_order.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    l.dv_realign_regions_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]
    l.dv_debruijn_build.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    l.dv_debruijn_destroy.argtypes = [C.c_void_p]
    l.dv_debruijn_destroy.restype = None
    l.dv_debruijn_kmer_size.argtypes = [C.c_void_p]
    l.dv_debruijn_haplotypes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    l.dv_debruijn_graphviz.argtypes = [C.c_void_p, C.c_void_p]
    l.dv_debruijn_compact_batch.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    l.dv_debruijn_compact_batch_device.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    l.dv_debruijn_compact_free.argtypes = [C.c_void_p]
    l.dv_debruijn_compact_free.restype = None
    l.dv_debruijn_device_last_stats.argtypes = [C.c_void_p]
    l.dv_debruijn_paths_batch.argtypes = l.dv_debruijn_compact_batch.argtypes
    l.dv_debruijn_paths_batch_device.argtypes = l.dv_debruijn_compact_batch_device.argtypes
    l.dv_debruijn_paths_free.argtypes = [C.c_void_p]
    l.dv_debruijn_paths_free.restype = None
    l.dv_debruijn_paths_last_stats.argtypes = [C.c_void_p]
    l.dv_debruijn_from_compact.argtypes = ([C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                            C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                            C.c_int32, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 7)
    l.dv_realign_regions.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    l.dv_realign_result_free.argtypes = [C.c_void_p]
    l.dv_realign_result_free.restype = None
    l.dv_phase_reads.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_char_p, C.c_int64, C.c_void_p,
                                 C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_int32]
    phase_batch = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                   C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                   C.c_void_p]
    l.dv_phase_reads_batch.argtypes = phase_batch
    l.dv_phase_reads_batch_device.argtypes = phase_batch + [C.c_void_p]
    l.dv_phase_device_last_stats.argtypes = [C.c_void_p]
    l.dv_count_alleles.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    l.dv_count_alleles_batch.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    l.dv_allele_counts_arrays.argtypes = [C.c_void_p] + [C.c_void_p] * 4
    l.dv_allele_counts_free.argtypes = [C.c_void_p]
    l.dv_allele_counts_free.restype = None
    l.dv_count_alleles_gvcf_batch.argtypes = [C.c_int32] + [C.c_void_p] * 7
    l.dv_gvcf_blocks_arrays.restype = C.c_int64
    l.dv_gvcf_blocks_arrays.argtypes = [C.c_void_p, C.c_void_p]
    l.dv_gvcf_blocks_free.argtypes = [C.c_void_p]
    l.dv_gvcf_blocks_free.restype = None
    l.dv_call_candidates_batch.argtypes = [C.c_int32] + [C.c_void_p] * 9
    l.dv_candidates_arrays.restype = C.c_int64
    l.dv_candidates_arrays.argtypes = [C.c_void_p] * 6
    l.dv_candidates_free.argtypes = [C.c_void_p]
    l.dv_candidates_free.restype = None
    l.dv_select_windows_batch.argtypes = [C.c_int32] + [C.c_void_p] * 7
    l.dv_windows_arrays.restype = C.c_int64
    l.dv_windows_arrays.argtypes = [C.c_void_p] * 5
    l.dv_windows_free.argtypes = [C.c_void_p]
    l.dv_windows_free.restype = None
    l.dv_count_batch_last_stats.argtypes = [C.c_void_p]
    l.dv_genotype_sites.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_double,
                                    C.c_int32, C.c_void_p]
    l.dv_genotype_sites_device.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                           C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    l.dv_genotypes_arrays.argtypes = [C.c_void_p, C.c_void_p]
    l.dv_genotypes_free.argtypes = [C.c_void_p]
    l.dv_genotypes_free.restype = None
    l.dv_genotype_min_nonref_prob.argtypes = [C.c_double]
    l.dv_genotype_min_nonref_prob.restype = C.c_double
    l.dv_genotype_device_last_stats.argtypes = [C.c_void_p]
    l.dv_gvcf_merge.argtypes = [C.c_int32] + [C.c_void_p] * 7
    l.dv_gvcf_merge_device.argtypes = [C.c_int32] + [C.c_void_p] * 8
    l.dv_gvcf_merged_arrays.argtypes = [C.c_void_p, C.c_void_p]
    l.dv_gvcf_merged_free.argtypes = [C.c_void_p]
    l.dv_gvcf_merged_free.restype = None
    l.dv_gvcf_merge_scan_chunk.argtypes = []
    l.dv_gvcf_merge_scan_chunk.restype = C.c_int32
    l.dv_gvcf_merge_last_stats.argtypes = [C.c_void_p]
    l.dv_gvcf_rows.argtypes = [C.c_void_p, C.c_void_p]
    l.dv_gvcf_rows_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    l.dv_gvcf_text_arrays.argtypes = [C.c_void_p, C.c_void_p]
    l.dv_gvcf_text_free.argtypes = [C.c_void_p]
    l.dv_gvcf_text_free.restype = None
    l.dv_gvcf_rows_last_stats.argtypes = [C.c_void_p]
    l.dv_bgzf_params.argtypes = [C.c_void_p]
    l.dv_bgzf_compress.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    l.dv_bgzf_compress_device.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    l.dv_bgzf_arrays.argtypes = [C.c_void_p, C.c_void_p]
    l.dv_bgzf_free.argtypes = [C.c_void_p]
    l.dv_bgzf_free.restype = None
    l.dv_bgzf_last_stats.argtypes = [C.c_void_p]
    l.dv_gvcf_rows_bgzf.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    l.dv_gvcf_rows_bgzf_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    l.dv_merge_alt_channels.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    _lib = l
  return _lib


def last_error() -> str:
  return lib().dv_last_error().decode()


def check(status: int):
  if status != DV_OK:
    raise DvError(status, last_error())


def try_crc32c(data: bytes) -> Optional[int]:
  if not os.path.exists(LIB_PATH):
    return None
  buf = bytes(data)
  return int(lib().dv_crc32c(buf, len(buf)))


def device_count() -> int:
  return int(lib().dv_device_count())
