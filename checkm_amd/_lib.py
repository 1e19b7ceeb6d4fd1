"""ctypes binding of libcheckm_hip.so (include/checkm_hip.h).

The library is the only compute path: if it is missing or no gfx950 device is usable this
module raises -- there is no CPU fallback anywhere in checkm_amd.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libcheckm_hip.so")

ABI_VERSION = 12
ENODEV = -4                 # CKM_ENODEV of include/checkm_hip.h: no usable HIP device


class CkmError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "libcheckm_hip error %d: %s" % (code, msg))
        self.code = code


class ModelHeader(C.Structure):
    _fields_ = [("name", C.c_char_p), ("acc", C.c_char_p), ("desc", C.c_char_p), ("leng", C.c_int32),
                ("has_ga", C.c_int32), ("has_tc", C.c_int32), ("has_nc", C.c_int32),
                ("ga", C.c_double * 2), ("tc", C.c_double * 2), ("nc", C.c_double * 2), ("evparam", C.c_float * 6), ("searchable", C.c_int32)]


class HitColumns(C.Structure):
    _fields_ = [("n", C.c_uint64), ("nbins", C.c_uint32), ("bin_row_off", C.POINTER(C.c_uint64)),
                ("seq", C.POINTER(C.c_uint32)), ("model", C.POINTER(C.c_uint32)),
                ("tlen", C.POINTER(C.c_int32)), ("qlen", C.POINTER(C.c_int32)),
                ("full_evalue", C.POINTER(C.c_double)), ("full_score", C.POINTER(C.c_float)), ("full_bias", C.POINTER(C.c_float)),
                ("dom_idx", C.POINTER(C.c_int32)), ("ndom", C.POINTER(C.c_int32)),
                ("c_evalue", C.POINTER(C.c_double)), ("i_evalue", C.POINTER(C.c_double)),
                ("dom_score", C.POINTER(C.c_float)), ("dom_bias", C.POINTER(C.c_float)),
                ("hmm_from", C.POINTER(C.c_int32)), ("hmm_to", C.POINTER(C.c_int32)),
                ("ali_from", C.POINTER(C.c_int32)), ("ali_to", C.POINTER(C.c_int32)),
                ("env_from", C.POINTER(C.c_int32)), ("env_to", C.POINTER(C.c_int32)), ("acc", C.POINTER(C.c_float)),
                ("target_name", C.POINTER(C.c_char_p)), ("full_score_d", C.POINTER(C.c_double)), ("dom_score_d", C.POINTER(C.c_double))]


HIT_FIELDS = ["seq", "model", "tlen", "qlen", "full_evalue", "full_score", "full_bias", "dom_idx", "ndom", "c_evalue",
              "i_evalue", "dom_score", "dom_bias", "hmm_from", "hmm_to", "ali_from", "ali_to", "env_from", "env_to", "acc"]


class SearchStats(C.Structure):
    _fields_ = [("pairs_ssv", C.c_uint64), ("pairs_msv_full", C.c_uint64), ("pairs_bias", C.c_uint64), ("pairs_vit", C.c_uint64),
                ("pairs_fwd", C.c_uint64), ("pairs_dom", C.c_uint64), ("envelopes", C.c_uint64), ("regions_multi", C.c_uint64), ("pairs_vit_exact", C.c_uint64), ("cells_ssv", C.c_uint64),
                ("residue_hmm", C.c_uint64), ("ms_ssv", C.c_double), ("ms_filters", C.c_double), ("ms_fwdbwd", C.c_double),
                ("ms_domains", C.c_double), ("ms_host", C.c_double), ("ms_total", C.c_double), ("ssv_launches", C.c_uint32), ("cascade_fallback_lanes", C.c_uint32),
                ("ws_cap_bytes", C.c_uint64), ("ws_used_bytes", C.c_uint64)]


class StageScores(C.Structure):
    _fields_ = [("msv_xJ", C.c_int32), ("msv_sc", C.c_float), ("null_sc", C.c_float), ("bias_sc", C.c_float),
                ("vit_xC", C.c_int32), ("vit_sc", C.c_float), ("fwd_sc", C.c_float), ("fwd_xC", C.c_float),
                ("fwd_nscale", C.c_int32), ("ssv_maxv", C.c_int32), ("msvp_xJ", C.c_int32), ("msvp_sc", C.c_float)]


class EnvelopeResult(C.Structure):
    _fields_ = [("envsc", C.c_float), ("oasc", C.c_float), ("fwd_xC", C.c_float), ("nscale", C.c_int32), ("null2", C.c_float * 20),
                ("hmm_from", C.c_int32), ("hmm_to", C.c_int32), ("ali_from", C.c_int32), ("ali_to", C.c_int32), ("ok", C.c_int32)]


class ModelInfo(C.Structure):
    _fields_ = [("nmodels", C.c_uint32), ("qlen", C.c_void_p), ("thr_kind", C.c_void_p), ("thr_full", C.c_void_p),
                ("thr_dom", C.c_void_p), ("is_pf", C.c_void_p), ("clan", C.c_void_p), ("nest_off", C.c_void_p),
                ("nest_idx", C.c_void_p), ("key", C.c_void_p)]


class ReduceFlags(C.Structure):
    _fields_ = [("ignore_thresholds", C.c_int32), ("skip_pseudogene_correction", C.c_int32), ("skip_adj_correction", C.c_int32),
                ("individual_markers", C.c_int32), ("evalue_threshold", C.c_double), ("length_threshold", C.c_double),
                ("bin_select", C.c_void_p), ("nvariants", C.c_uint32), ("bin_variant", C.c_void_p)]


class MarkerSetsCSR(C.Structure):
    _fields_ = [("nbins", C.c_uint32), ("set_off", C.c_void_p), ("marker_off", C.c_void_p), ("marker_key", C.c_void_p)]


class QAColumns(C.Structure):
    _fields_ = [("nbins", C.c_uint32), ("hist", C.POINTER(C.c_int32)), ("completeness", C.POINTER(C.c_double)),
                ("contamination", C.POINTER(C.c_double)), ("set_off", C.POINTER(C.c_uint32)),
                ("set_present", C.POINTER(C.c_int32)), ("set_multi", C.POINTER(C.c_int32)),
                ("nkept", C.c_uint64), ("kept_bin_off", C.POINTER(C.c_uint64)), ("kept_key", C.POINTER(C.c_uint32)),
                ("kept_row", C.POINTER(C.c_uint64)), ("kept_row2", C.POINTER(C.c_uint64)),
                ("kept_tlen", C.POINTER(C.c_int32)), ("kept_hmm_from", C.POINTER(C.c_int32)), ("kept_hmm_to", C.POINTER(C.c_int32)),
                ("kept_ali_from", C.POINTER(C.c_int32)), ("kept_ali_to", C.POINTER(C.c_int32)),
                ("kept_env_from", C.POINTER(C.c_int32)), ("kept_env_to", C.POINTER(C.c_int32))]


class OrfColumns(C.Structure):
    _fields_ = [("n", C.c_uint64), ("contig", C.POINTER(C.c_uint32)), ("ndx", C.POINTER(C.c_int32)), ("stop_val", C.POINTER(C.c_int32)),
                ("type", C.POINTER(C.c_uint8)), ("strand_rev", C.POINTER(C.c_uint8)), ("edge", C.POINTER(C.c_uint8)),
                ("ms_flags", C.c_double), ("ms_chain", C.c_double), ("bases", C.c_uint64), ("padded_bytes", C.c_uint64)]


class NucBatchView(C.Structure):
    _fields_ = [("text", C.c_void_p), ("contig_off", C.POINTER(C.c_uint64)), ("bin_first", C.POINTER(C.c_uint32)), ("contig_ids", C.c_void_p),
                ("bin_bases", C.POINTER(C.c_uint64)), ("ncontigs", C.c_uint32), ("nbins", C.c_uint32)]


class NucSeqView(C.Structure):
    _fields_ = [("text", C.c_void_p), ("text_bytes", C.c_uint64), ("seq_off", C.POINTER(C.c_uint64)), ("seq_bytes", C.POINTER(C.c_uint64)),
                ("file_first", C.POINTER(C.c_uint32)), ("seq_ids", C.POINTER(C.c_char_p)), ("nseq", C.c_uint32), ("nfiles", C.c_uint32)]


class NucStatsColumns(C.Structure):
    _fields_ = [("nseq", C.c_uint32), ("count", C.POINTER(C.c_uint64)), ("piece_off", C.POINTER(C.c_uint64)), ("piece_len", C.POINTER(C.c_uint64)),
                ("tetra", C.POINTER(C.c_uint32)), ("bytes", C.c_uint64), ("tiles", C.c_uint64), ("run_starts", C.c_uint64),
                ("ms_upload", C.c_double), ("ms_count", C.c_double), ("ms_fill", C.c_double), ("ms_total", C.c_double)]


class TetraProfileView(C.Structure):
    _fields_ = [("n", C.c_uint32), ("ids", C.POINTER(C.c_char_p)), ("sig", C.POINTER(C.c_double))]


class OutlierBounds(C.Structure):
    _fields_ = [("ntables", C.c_uint32), ("tab_off", C.c_void_p), ("key", C.c_void_p), ("lo", C.c_void_p), ("hi", C.c_void_p),
                ("bin_gc_tab", C.c_void_p), ("bin_cd_tab", C.c_void_p), ("td_tab", C.c_uint32)]


class OutlierColumns(C.Structure):
    _fields_ = [("nseq", C.c_uint32), ("nbins", C.c_uint32)] + [(f, C.POINTER(C.c_double)) for f in ("gc", "delta_gc", "cd", "delta_cd", "td", "weight")] + \
               [("flags", C.POINTER(C.c_uint8)), ("mean_gc", C.POINTER(C.c_double)), ("mean_cd", C.POINTER(C.c_double)), ("bin_sig", C.POINTER(C.c_double))] + \
               [(f, C.c_double) for f in ("ms_upload", "ms_seq", "ms_binsig", "ms_td", "ms_flags", "ms_total")]


class MergeColumns(C.Structure):
    _fields_ = [("npairs", C.c_uint64), ("compared", C.c_uint64), ("nbatches", C.c_uint64), ("kept", C.c_int32),
                ("i", C.POINTER(C.c_uint32)), ("j", C.POINTER(C.c_uint32)), ("col", C.POINTER(C.c_double) * 9)] + \
               [(f, C.c_double) for f in ("ms_upload", "ms_bins", "ms_count", "ms_scan", "ms_fill", "ms_download", "ms_write", "ms_total")]


class BamHeaderView(C.Structure):
    _fields_ = [("n_ref", C.c_uint32), ("names", C.POINTER(C.c_char_p)), ("lengths", C.POINTER(C.c_int64)), ("header_bytes", C.c_uint64)]


class CoverageParams(C.Structure):
    _fields_ = [("min_align_per", C.c_double), ("max_edit_dist_per", C.c_double), ("min_qc", C.c_double), ("all_reads", C.c_int32), ("budget_bytes", C.c_uint64)]


class CoverageTiming(C.Structure):
    _fields_ = [("records", C.c_uint64), ("batches", C.c_uint64), ("blocks", C.c_uint64), ("inflated_bytes", C.c_uint64),
                ("error_reason", C.c_uint32), ("error_record", C.c_uint64), ("error_read", C.c_char * 256)] + \
               [(f, C.c_double) for f in ("ms_read", "ms_inflate", "ms_offsets", "ms_upload", "ms_kernel", "ms_download", "ms_total")]


class CoverageWindowsParams(C.Structure):
    _fields_ = [("min_align_per", C.c_double), ("max_edit_dist_per", C.c_double), ("all_reads", C.c_int32), ("window_size", C.c_int64), ("budget_bytes", C.c_uint64)]


class CoverageWindowsTiming(C.Structure):
    _fields_ = CoverageTiming._fields_ + [("ms_scan", C.c_double), ("slots", C.c_uint64)]


class SeqWindowsTiming(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("windows", "pieces", "batches", "bytes", "skipped_seqs")] + \
               [(f, C.c_double) for f in ("ms_upload", "ms_count", "ms_td", "ms_download", "ms_total")]


class RefDistTiming(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("windows", "blocks", "batches", "bytes")] + \
               [(f, C.c_double) for f in ("ms_scaffold", "ms_upload", "ms_blocks", "ms_scan", "ms_windows", "ms_download", "ms_total")]


class FastaIdsView(C.Structure):
    _fields_ = [("seq_ids", C.POINTER(C.c_char_p)), ("seq_bytes", C.POINTER(C.c_uint64)), ("seq_cp", C.POINTER(C.c_uint64)), ("file_first", C.POINTER(C.c_uint32)),
                ("nseq", C.c_uint32), ("nfiles", C.c_uint32)]


class UnbinnedTotals(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("binned_ids", "binned_bases", "all_seqs", "all_bases", "unbinned_seqs", "unbinned_bases")]


class UnbinnedTiming(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("kept", "tiles", "batches", "bytes")] + \
               [(f, C.c_double) for f in ("ms_stage", "ms_upload", "ms_count", "ms_sum", "ms_download", "ms_total")]


class AaiColumns(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("ngroups", "npairs", "nbatches", "bytes")] + \
               [("pair_off", C.POINTER(C.c_uint64)), ("mismatches", C.POINTER(C.c_int32)), ("compared", C.POINTER(C.c_int32)), ("aai", C.POINTER(C.c_double))] + \
               [(f, C.c_double) for f in ("ms_pack", "ms_upload", "ms_kernel", "ms_download", "ms_total")]


class MsetColumns(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("nqueries", "nfamilies", "npairs", "nbatches", "nrounds", "tests")] + \
               [("flag", C.POINTER(C.c_uint8)), ("counts", C.POINTER(C.c_uint32)), ("pair_off", C.POINTER(C.c_uint64)),
                ("i", C.POINTER(C.c_uint32)), ("j", C.POINTER(C.c_uint32)), ("count", C.POINTER(C.c_uint32))] + \
               [(f, C.c_double) for f in ("ms_upload", "ms_markers", "ms_pack", "ms_count", "ms_scan", "ms_fill", "ms_download", "ms_total")]


class SimArgs(C.Structure):
    _fields_ = [("nmarkers", C.c_uint32), ("key_off", C.c_void_p), ("key", C.c_void_p), ("nkeys", C.c_uint64),
                ("nsets", C.c_uint32), ("ms_off", C.c_void_p), ("cs_off", C.c_void_p), ("ncs", C.c_uint64), ("cs_marker", C.c_void_p), ("nmembers", C.c_uint64),
                ("nreplicates", C.c_uint32), ("rs_off", C.c_void_p), ("starts", C.c_void_p), ("nstarts", C.c_uint64), ("contig_len", C.c_void_p)]


class SimInfo(C.Structure):
    _fields_ = [("nrounds", C.c_uint64)] + [(f, C.c_double) for f in ("ms_pack", "ms_upload", "ms_kernel", "ms_download", "ms_total")]


class SimScafArgs(C.Structure):
    _fields_ = [("ngenomes", C.c_uint32), ("nscaf", C.c_void_p), ("nmarkers", C.c_uint32), ("sc_off", C.c_void_p), ("sc", C.c_void_p), ("nsc", C.c_uint64),
                ("nsets", C.c_uint32), ("ms_off", C.c_void_p), ("cs_off", C.c_void_p), ("ncs", C.c_uint64), ("cs_marker", C.c_void_p), ("nmembers", C.c_uint64),
                ("nreplicates", C.c_uint32), ("test", C.c_void_p), ("cont", C.c_void_p), ("bit_off", C.c_void_p), ("bits", C.c_void_p), ("nwords", C.c_uint64)]


class SelectArgs(C.Structure):
    _fields_ = [("ngenomes", C.c_uint32), ("genome_len", C.c_void_p), ("nmarkers", C.c_uint32), ("key_off", C.c_void_p), ("key", C.c_void_p), ("nkeys", C.c_uint64),
                ("nsets", C.c_uint32), ("ms_off", C.c_void_p), ("cs_off", C.c_void_p), ("ncs", C.c_uint64), ("cs_marker", C.c_void_p), ("nmembers", C.c_uint64),
                ("nreplicates", C.c_uint32), ("contig_len", C.c_int64), ("comp_lo", C.c_double), ("comp_hi", C.c_double), ("cont_lo", C.c_double), ("cont_hi", C.c_double),
                ("seed", C.c_uint64)]


class SelectOut(C.Structure):
    _fields_ = [("truth", C.c_void_p), ("out", C.c_void_p), ("rows", C.c_void_p)]


class PlaceArgs(C.Structure):
    _fields_ = [("nnodes", C.c_uint32), ("child_off", C.c_void_p), ("child", C.c_void_p), ("nchild", C.c_uint64), ("length", C.c_void_p),
                ("nsites", C.c_uint32), ("nrows", C.c_uint32), ("row_off", C.c_void_p), ("rows", C.c_void_p), ("nrow_bytes", C.c_uint64),
                ("nqueries", C.c_uint32), ("q_off", C.c_void_p), ("queries", C.c_void_p), ("nquery_bytes", C.c_uint64),
                ("nrates", C.c_uint32), ("weights", C.c_void_p), ("U", C.c_void_p), ("Uinv", C.c_void_p), ("pi", C.c_void_p),
                ("exp_len", C.c_void_p), ("exp_half", C.c_void_p), ("nfrac", C.c_uint32), ("exp_dist", C.c_void_p),
                ("npend", C.c_uint32), ("exp_pend", C.c_void_p), ("max_pitches", C.c_uint32)]


class PlaceOut(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in ("top_edge", "scan_m", "scan_e", "ref_m", "ref_e", "ref_f", "ref_g")]


_PLACE_MS = ("ms_pack", "ms_upload", "ms_matrices", "ms_sweeps", "ms_tables", "ms_scan", "ms_topk", "ms_refine", "ms_download", "ms_total")


class PlaceInfo(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("nchunks", "chunk_sites", "nlevels_up", "nlevels_down")] + [(f, C.c_double) for f in _PLACE_MS]


class NhmmArgs(C.Structure):
    _fields_ = [("nmodels", C.c_uint32), ("M", C.c_void_p), ("tab_off", C.c_void_p), ("emis", C.c_void_p), ("trans", C.c_void_p), ("ntab", C.c_uint64),
                ("min_score", C.c_void_p), ("stride", C.c_uint32), ("overlap", C.c_uint32), ("strands", C.c_uint32)]


_NHMM_ROWS = ("row_model", "row_seq", "row_strand", "row_pos", "row_start", "row_score")
_NHMM_HITS = ("hit_model", "hit_seq", "hit_strand", "hit_from", "hit_to", "hit_score")


class NhmmColumns(C.Structure):
    _fields_ = [("nrows", C.c_uint64)] + [(f, C.c_void_p) for f in _NHMM_ROWS] + [("nhits", C.c_uint64)] + [(f, C.c_void_p) for f in _NHMM_HITS]


_NHMM_MS = ("ms_tables", "ms_upload", "ms_scan", "ms_compact", "ms_download", "ms_hits", "ms_total")


class NhmmInfo(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("tiles", "launches", "cells", "batches")] + [(f, C.c_double) for f in _NHMM_MS]


class GtreeArgs(C.Structure):
    _fields_ = [("nrows", C.c_uint32), ("ncols", C.c_uint32), ("text", C.c_void_p), ("ntext_bytes", C.c_uint64), ("nreps", C.c_uint32), ("cols", C.c_void_p),
                ("base", C.c_uint32), ("model", C.c_int32), ("max_dist", C.c_double), ("matrix", C.c_void_p), ("nmatrices", C.c_uint32)]


class GtreeOut(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in ("compared", "differ", "dist", "merge_ij", "merge_len")]


_GTREE_MS = ("ms_upload", "ms_gather", "ms_counts", "ms_dist", "ms_joins", "ms_download", "ms_total")


class GtreeInfo(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("nrounds", "ntrees", "launches")] + [(f, C.c_double) for f in _GTREE_MS]


class GenetreeArgs(C.Structure):
    _fields_ = [("ntrees", C.c_uint32)] + [(f, C.c_void_p) for f in ("node_off", "leaf_off", "class_off", "group_off", "gpair_off", "first", "last", "parent", "length", "internal",
                                                                     "leaf_genome", "leaf_species", "leaf_class", "class_total", "pair_a", "pair_b")]


class GenetreeOut(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in ("consistency", "pair_flag", "group_node", "group_mixed")]


_GENETREE_MS = ("ms_upload", "ms_consistency", "ms_flags", "ms_conspecific", "ms_download", "ms_total")


class GenetreeInfo(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("nrounds", "ntrees", "launches")] + [(f, C.c_double) for f in _GENETREE_MS]


class NearidArgs(C.Structure):
    _fields_ = [("text", C.c_void_p), ("n_rows", C.c_uint32), ("row_len", C.c_uint32), ("row_stride", C.c_uint32), ("limit", C.c_void_p)]


class NearidOut(C.Structure):
    _fields_ = [("near", C.c_void_p)]


_NEARID_MS = ("ms_upload", "ms_kernel", "ms_download", "ms_total")


class NearidInfo(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("nbands", "npairs", "launches", "blocks")] + [(f, C.c_double) for f in _NEARID_MS]


class GeneColumns(C.Structure):
    _fields_ = [("n", C.c_uint64), ("bin", C.POINTER(C.c_uint32)), ("contig", C.POINTER(C.c_uint32)), ("begin", C.POINTER(C.c_int32)), ("end", C.POINTER(C.c_int32)),
                ("strand", C.POINTER(C.c_int8)), ("start_type", C.POINTER(C.c_uint8)), ("partial_left", C.POINTER(C.c_uint8)), ("partial_right", C.POINTER(C.c_uint8)),
                ("rbs_bin", C.POINTER(C.c_int32)), ("mot_len", C.POINTER(C.c_int32)), ("mot_ndx", C.POINTER(C.c_int32)), ("mot_spacer", C.POINTER(C.c_int32)),
                ("gc_cont", C.POINTER(C.c_double)), ("conf", C.POINTER(C.c_double)), ("score", C.POINTER(C.c_double)), ("cscore", C.POINTER(C.c_double)),
                ("sscore", C.POINTER(C.c_double)), ("rscore", C.POINTER(C.c_double)), ("uscore", C.POINTER(C.c_double)), ("tscore", C.POINTER(C.c_double)),
                ("prot_off", C.POINTER(C.c_uint64)), ("prot", C.POINTER(C.c_char)),
                ("nbins", C.c_uint64), ("bin_trained", C.POINTER(C.c_uint8)), ("bin_uses_sd", C.POINTER(C.c_uint8)), ("bin_gc", C.POINTER(C.c_double)),
                ("bin_bases", C.POINTER(C.c_uint64)), ("bin_coding", C.POINTER(C.c_uint64)), ("bin_nodes", C.POINTER(C.c_uint64)),
                ("ms_nodes", C.c_double), ("ms_dp_train", C.c_double), ("ms_score", C.c_double), ("ms_dp_find", C.c_double), ("ms_total", C.c_double)]


class TableColumns(C.Structure):
    _fields_ = [("cols", HitColumns), ("target_accession", C.POINTER(C.c_char_p)), ("query_name", C.POINTER(C.c_char_p)),
                ("query_accession", C.POINTER(C.c_char_p)), ("description", C.POINTER(C.c_char_p)),
                ("full_bias_d", C.POINTER(C.c_double)), ("dom_bias_d", C.POINTER(C.c_double)), ("acc_d", C.POINTER(C.c_double)),
                ("bin_missing", C.POINTER(C.c_uint8))]


# every symbol include/checkm_hip.h declares
EXPORTS = ["ckm_last_error", "ckm_abi_version", "ckm_device_count", "ckm_ctx_create", "ckm_ctx_destroy", "ckm_ctx_reserve",
           "ckm_profiles_load", "ckm_profiles_count", "ckm_profiles_header", "ckm_profiles_free",
           "ckm_seqs_pack", "ckm_seqs_from_fasta", "ckm_seqs_count", "ckm_seqs_bin_offsets", "ckm_seqs_name", "ckm_seqs_residues", "ckm_seqs_free", "ckm_search", "ckm_hits_columns", "ckm_hits_free",
           "ckm_hits_write_domtblout", "ckm_hits_write_alignments", "ckm_last_search_stats", "ckm_reduce", "ckm_qa_columns_get", "ckm_qa_free", "ckm_count_sets",
           "ckm_align", "ckm_tables_read", "ckm_tables_assign_models", "ckm_tables_get", "ckm_tables_free",
           "ckm_orf_scan", "ckm_orf_columns_get", "ckm_orf_free", "ckm_debug_orf_flags", "ckm_genes_call", "ckm_genes_columns_get", "ckm_genes_free", "ckm_genes_coding_union", "ckm_genes_write_bin",
           "ckm_nuc_batch_read", "ckm_nuc_batch_view_get", "ckm_nuc_batch_free",
           "ckm_nucseq_read", "ckm_nucseq_view_get", "ckm_nucseq_free", "ckm_nucstats_run", "ckm_nucstats_columns_get", "ckm_nucstats_free", "ckm_bin_genes_read",
           "ckm_seq_genes_read", "ckm_tetra_profile_read", "ckm_tetra_profile_view_get", "ckm_tetra_profile_gather", "ckm_tetra_profile_free",
           "ckm_outliers_run", "ckm_outliers_columns_get", "ckm_outliers_free",
           "ckm_merge_check", "ckm_merge_run", "ckm_merge_columns_get", "ckm_merge_free",
           "ckm_bam_open", "ckm_bam_header", "ckm_bam_close", "ckm_coverage_check", "ckm_coverage_run",
           "ckm_coverage_windows_check", "ckm_coverage_windows_layout", "ckm_coverage_windows_run",
           "ckm_seq_windows_layout", "ckm_seq_windows_run", "ckm_seq_windows_coding",
           "ckm_refdist_check", "ckm_refdist_run", "ckm_refdist_coding",
           "ckm_fasta_ids_read", "ckm_fasta_ids_view_get", "ckm_fasta_ids_free", "ckm_unbinned_select", "ckm_unbinned_count", "ckm_unbinned_write",
           "ckm_aai_check", "ckm_aai_run", "ckm_aai_columns_get", "ckm_aai_free",
           "ckm_mset_check", "ckm_mset_table_create", "ckm_mset_table_free", "ckm_mset_markers", "ckm_mset_colocated", "ckm_mset_columns_get", "ckm_mset_result_free",
           "ckm_sim_check", "ckm_sim_run", "ckm_simscaf_check", "ckm_simscaf_run", "ckm_select_check", "ckm_select_run", "ckm_place_check", "ckm_place_run",
           "ckm_nhmm_check", "ckm_nhmm_run", "ckm_nhmm_columns_get", "ckm_nhmm_free", "ckm_gtree_check", "ckm_gtree_host", "ckm_gtree_run",
           "ckm_genetree_check", "ckm_genetree_host", "ckm_genetree_run", "ckm_nearid_check", "ckm_nearid_host", "ckm_nearid_run",
           "ckm_debug_stages", "ckm_debug_ssv", "ckm_debug_filters", "ckm_debug_envelopes", "ckm_debug_envelope_paths", "ckm_debug_region"]

_lib = None


def load():
    """Load the shared library (no device needed for this); raises if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    L.ckm_last_error.restype = C.c_char_p
    L.ckm_device_count.argtypes = [C.POINTER(C.c_int)]
    L.ckm_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.ckm_ctx_destroy.argtypes = [C.c_void_p]
    L.ckm_ctx_destroy.restype = None
    L.ckm_ctx_reserve.argtypes = [C.c_void_p, C.c_uint64, C.c_double]
    L.ckm_profiles_load.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p)]
    L.ckm_profiles_count.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.ckm_profiles_header.argtypes = [C.c_void_p, C.c_int32, C.POINTER(ModelHeader)]
    L.ckm_profiles_free.argtypes = [C.c_void_p]
    L.ckm_profiles_free.restype = None
    L.ckm_seqs_pack.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_void_p)]
    L.ckm_seqs_from_fasta.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_void_p)]
    L.ckm_seqs_count.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.ckm_seqs_bin_offsets.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint32))]
    L.ckm_seqs_name.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_int32)]
    L.ckm_seqs_residues.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.ckm_seqs_free.argtypes = [C.c_void_p]
    L.ckm_seqs_free.restype = None
    L.ckm_search.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                             C.POINTER(C.c_void_p)]
    L.ckm_hits_columns.argtypes = [C.c_void_p, C.POINTER(HitColumns)]
    L.ckm_hits_free.argtypes = [C.c_void_p]
    L.ckm_hits_free.restype = None
    L.ckm_hits_write_domtblout.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p]
    L.ckm_hits_write_alignments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p]
    L.ckm_last_search_stats.argtypes = [C.c_void_p, C.POINTER(SearchStats)]
    L.ckm_reduce.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(HitColumns), C.c_void_p, C.POINTER(ModelInfo),
                             C.POINTER(ReduceFlags), C.POINTER(MarkerSetsCSR), C.POINTER(C.c_void_p)]
    L.ckm_qa_columns_get.argtypes = [C.c_void_p, C.POINTER(QAColumns)]
    L.ckm_qa_free.argtypes = [C.c_void_p]
    L.ckm_qa_free.restype = None
    L.ckm_count_sets.argtypes = [C.c_void_p, C.POINTER(MarkerSetsCSR)] + [C.c_void_p] * 7
    L.ckm_align.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.ckm_tables_read.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_void_p)]
    L.ckm_tables_assign_models.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_uint64)]
    L.ckm_tables_get.argtypes = [C.c_void_p, C.POINTER(TableColumns)]
    L.ckm_tables_free.argtypes = [C.c_void_p]
    L.ckm_tables_free.restype = None
    L.ckm_orf_scan.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.ckm_orf_columns_get.argtypes = [C.c_void_p, C.POINTER(OrfColumns)]
    L.ckm_orf_free.argtypes = [C.c_void_p]
    L.ckm_orf_free.restype = None
    L.ckm_genes_call.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.ckm_genes_columns_get.argtypes = [C.c_void_p, C.POINTER(GeneColumns)]
    L.ckm_genes_free.argtypes = [C.c_void_p]
    L.ckm_genes_free.restype = None
    L.ckm_genes_coding_union.argtypes = [C.c_void_p, C.c_void_p]
    L.ckm_genes_write_bin.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p]
    L.ckm_nuc_batch_read.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_void_p)]
    L.ckm_nuc_batch_view_get.argtypes = [C.c_void_p, C.POINTER(NucBatchView)]
    L.ckm_nuc_batch_free.argtypes = [C.c_void_p]
    L.ckm_nuc_batch_free.restype = None
    L.ckm_nucseq_read.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_void_p)]
    L.ckm_nucseq_view_get.argtypes = [C.c_void_p, C.POINTER(NucSeqView)]
    L.ckm_nucseq_free.argtypes = [C.c_void_p]
    L.ckm_nucseq_free.restype = None
    L.ckm_nucstats_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]
    L.ckm_nucstats_columns_get.argtypes = [C.c_void_p, C.POINTER(NucStatsColumns)]
    L.ckm_nucstats_free.argtypes = [C.c_void_p]
    L.ckm_nucstats_free.restype = None
    L.ckm_bin_genes_read.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ckm_seq_genes_read.argtypes = [C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, C.c_void_p]
    L.ckm_tetra_profile_read.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    L.ckm_tetra_profile_view_get.argtypes = [C.c_void_p, C.POINTER(TetraProfileView)]
    L.ckm_tetra_profile_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    L.ckm_tetra_profile_free.argtypes = [C.c_void_p]
    L.ckm_tetra_profile_free.restype = None
    L.ckm_outliers_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(OutlierBounds), C.POINTER(C.c_int64), C.POINTER(C.c_void_p)]
    L.ckm_outliers_columns_get.argtypes = [C.c_void_p, C.POINTER(OutlierColumns)]
    L.ckm_outliers_free.argtypes = [C.c_void_p]
    L.ckm_outliers_free.restype = None
    L.ckm_merge_check.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ckm_merge_run.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p), C.c_char_p, C.c_uint64, C.c_int,
                                C.POINTER(C.c_void_p)]
    L.ckm_merge_columns_get.argtypes = [C.c_void_p, C.POINTER(MergeColumns)]
    L.ckm_merge_free.argtypes = [C.c_void_p]
    L.ckm_merge_free.restype = None
    L.ckm_bam_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    L.ckm_bam_header.argtypes = [C.c_void_p, C.POINTER(BamHeaderView)]
    L.ckm_bam_close.argtypes = [C.c_void_p]
    L.ckm_bam_close.restype = None
    L.ckm_coverage_check.argtypes = [C.POINTER(CoverageParams)]
    L.ckm_coverage_run.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CoverageParams), C.c_void_p, C.POINTER(CoverageTiming)]
    L.ckm_coverage_windows_check.argtypes = [C.POINTER(CoverageWindowsParams)]
    L.ckm_coverage_windows_layout.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.ckm_coverage_windows_run.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CoverageWindowsParams), C.c_void_p, C.c_void_p, C.POINTER(CoverageWindowsTiming)]
    L.ckm_seq_windows_layout.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.ckm_seq_windows_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.POINTER(SeqWindowsTiming)]
    L.ckm_seq_windows_coding.argtypes = [C.POINTER(C.c_char_p), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.ckm_refdist_check.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]
    L.ckm_refdist_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.POINTER(RefDistTiming)]
    L.ckm_refdist_coding.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_int64)]
    L.ckm_fasta_ids_read.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_void_p)]
    L.ckm_fasta_ids_view_get.argtypes = [C.c_void_p, C.POINTER(FastaIdsView)]
    L.ckm_fasta_ids_free.argtypes = [C.c_void_p]
    L.ckm_fasta_ids_free.restype = None
    L.ckm_unbinned_select.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(UnbinnedTotals)]
    L.ckm_unbinned_count.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.POINTER(UnbinnedTiming)]
    L.ckm_unbinned_write.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_int64)]
    L.ckm_aai_check.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ckm_aai_run.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
    L.ckm_aai_columns_get.argtypes = [C.c_void_p, C.POINTER(AaiColumns)]
    L.ckm_aai_free.argtypes = [C.c_void_p]
    L.ckm_aai_free.restype = None
    L.ckm_mset_check.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double]
    L.ckm_mset_table_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_void_p)]
    L.ckm_mset_table_free.argtypes = [C.c_void_p]
    L.ckm_mset_table_free.restype = None
    L.ckm_mset_markers.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]
    L.ckm_mset_colocated.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_uint64,
                                     C.POINTER(C.c_void_p)]
    L.ckm_mset_columns_get.argtypes = [C.c_void_p, C.POINTER(MsetColumns)]
    L.ckm_mset_result_free.argtypes = [C.c_void_p]
    L.ckm_mset_result_free.restype = None
    L.ckm_sim_check.argtypes = [C.POINTER(SimArgs)]
    L.ckm_sim_run.argtypes = [C.c_void_p, C.POINTER(SimArgs), C.c_uint64, C.c_void_p, C.POINTER(SimInfo)]
    L.ckm_simscaf_check.argtypes = [C.POINTER(SimScafArgs)]
    L.ckm_simscaf_run.argtypes = [C.c_void_p, C.POINTER(SimScafArgs), C.c_uint64, C.c_void_p, C.POINTER(SimInfo)]
    L.ckm_select_check.argtypes = [C.POINTER(SelectArgs)]
    L.ckm_select_run.argtypes = [C.c_void_p, C.POINTER(SelectArgs), C.c_uint64, C.POINTER(SelectOut), C.POINTER(SimInfo)]
    L.ckm_place_check.argtypes = [C.POINTER(PlaceArgs)]
    L.ckm_place_run.argtypes = [C.c_void_p, C.POINTER(PlaceArgs), C.c_uint64, C.POINTER(PlaceOut), C.POINTER(PlaceInfo)]
    L.ckm_nhmm_check.argtypes = [C.POINTER(NhmmArgs)]
    L.ckm_nhmm_run.argtypes = [C.c_void_p, C.POINTER(NhmmArgs), C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(NhmmInfo)]
    L.ckm_nhmm_columns_get.argtypes = [C.c_void_p, C.POINTER(NhmmColumns)]
    L.ckm_nhmm_free.argtypes = [C.c_void_p]
    L.ckm_nhmm_free.restype = None
    L.ckm_gtree_check.argtypes = [C.POINTER(GtreeArgs)]
    L.ckm_gtree_host.argtypes = [C.POINTER(GtreeArgs), C.c_uint64, C.POINTER(GtreeOut), C.POINTER(GtreeInfo)]
    L.ckm_gtree_run.argtypes = [C.c_void_p, C.POINTER(GtreeArgs), C.c_uint64, C.POINTER(GtreeOut), C.POINTER(GtreeInfo)]
    L.ckm_genetree_check.argtypes = [C.POINTER(GenetreeArgs)]
    L.ckm_genetree_host.argtypes = [C.POINTER(GenetreeArgs), C.c_uint64, C.POINTER(GenetreeOut), C.POINTER(GenetreeInfo)]
    L.ckm_genetree_run.argtypes = [C.c_void_p, C.POINTER(GenetreeArgs), C.c_uint64, C.POINTER(GenetreeOut), C.POINTER(GenetreeInfo)]
    L.ckm_nearid_check.argtypes = [C.POINTER(NearidArgs)]
    L.ckm_nearid_host.argtypes = [C.POINTER(NearidArgs), C.c_uint64, C.POINTER(NearidOut), C.POINTER(NearidInfo)]
    L.ckm_nearid_run.argtypes = [C.c_void_p, C.POINTER(NearidArgs), C.c_uint64, C.POINTER(NearidOut), C.POINTER(NearidInfo)]
    L.ckm_debug_orf_flags.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_double)]
    L.ckm_debug_stages.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.ckm_debug_ssv.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p]
    L.ckm_debug_filters.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_uint32,
                                    C.c_void_p, C.POINTER(C.c_uint32)]
    L.ckm_debug_envelopes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_uint32, C.c_void_p]
    L.ckm_debug_envelope_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ckm_debug_region.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    if L.ckm_abi_version() != ABI_VERSION:
        raise ImportError("libcheckm_hip ABI version mismatch")
    _lib = L
    return L


def _chk(rc):
    if rc != 0:
        raise CkmError(rc, load().ckm_last_error().decode(errors="replace"))


def device_count():
    n = C.c_int(0)
    rc = load().ckm_device_count(C.byref(n))
    return n.value if rc == 0 else 0


class Context(object):
    def __init__(self, device=0):
        self.h = C.c_void_p()
        _chk(load().ckm_ctx_create(device, C.byref(self.h)))
        self.device = device

    def close(self):
        if self.h:
            load().ckm_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def reserve(self, pairs, cells):
        """Start allocating the workspace a search of that size will ask for, in the background (ckm_ctx_reserve: `cells` = sum over
        the bins, over the models a bin is scanned against, of (Mp + 64) * Mp, Mp the model length padded to 64)."""
        _chk(load().ckm_ctx_reserve(self.h, int(pairs), float(cells)))

    def stats(self):
        st = SearchStats()
        _chk(load().ckm_last_search_stats(self.h, C.byref(st)))
        return st


class Profiles(object):
    def __init__(self, ctx, path):
        self.ctx = ctx
        self.h = C.c_void_p()
        _chk(load().ckm_profiles_load(ctx.h, path.encode(), C.byref(self.h)))
        n = C.c_int32()
        _chk(load().ckm_profiles_count(self.h, C.byref(n)))
        self.n = n.value
        self.headers = []
        for i in range(self.n):
            hd = ModelHeader()
            _chk(load().ckm_profiles_header(self.h, i, C.byref(hd)))
            self.headers.append({"name": hd.name.decode(), "acc": hd.acc.decode() if hd.acc else None,
                                 "desc": hd.desc.decode() if hd.desc else None, "leng": hd.leng,
                                 "ga": tuple(hd.ga) if hd.has_ga else None, "tc": tuple(hd.tc) if hd.has_tc else None,
                                 "nc": tuple(hd.nc) if hd.has_nc else None, "evparam": tuple(hd.evparam), "searchable": bool(hd.searchable)})

    def close(self):
        if self.h:
            load().ckm_profiles_free(self.h)
            self.h = C.c_void_p()


class _LazyStrings(object):
    """names[i] / descs[i] fetched from the library on demand (millions of ORFs need no Python list)."""

    def __init__(self, seqs, which):
        self.seqs, self.which, self.cache = seqs, which, {}

    def __len__(self):
        return self.seqs.nseq

    def __getitem__(self, i):
        v = self.cache.get(i)
        if v is None:
            name, desc = C.c_char_p(), C.c_char_p()
            _chk(load().ckm_seqs_name(self.seqs.h, int(i), C.byref(name), C.byref(desc), None))
            v = (name.value if self.which == 0 else desc.value).decode()
            self.cache[i] = v
        return v


class Seqs(object):
    """All sequences of all bins, packed and resident in HBM."""

    @classmethod
    def from_fasta(cls, ctx, paths):
        """One protein FASTA file per bin, read, digitized and packed by the library (ckm_seqs_from_fasta)."""
        self = cls.__new__(cls)
        self.ctx = ctx
        arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
        self.h = C.c_void_p()
        _chk(load().ckm_seqs_from_fasta(ctx.h, arr, len(paths), C.byref(self.h)))
        n, nb = C.c_uint32(), C.c_uint32()
        _chk(load().ckm_seqs_count(self.h, C.byref(n), C.byref(nb)))
        self.nseq, self.nbins = n.value, nb.value
        bo = C.POINTER(C.c_uint32)()
        _chk(load().ckm_seqs_bin_offsets(self.h, C.byref(bo)))
        self.bin_off = np.ctypeslib.as_array(bo, shape=(self.nbins + 1,)).copy()
        tot = C.c_uint64()
        _chk(load().ckm_seqs_residues(self.h, C.byref(tot)))
        self.total_residues = int(tot.value)
        self.names = _LazyStrings(self, 0)
        self.descs = _LazyStrings(self, 1)
        return self

    def __init__(self, ctx, bins):
        """bins: list of lists of (name, desc, residues) records."""
        self.ctx = ctx
        names, descs, parts = [], [], []
        bin_off = [0]
        for recs in bins:
            for name, desc, seq in recs:
                names.append(name.encode())
                descs.append((desc or "").encode())
                parts.append(seq.encode() if isinstance(seq, str) else seq)
            bin_off.append(len(names))
        self.nseq = len(names)
        self.nbins = len(bins)
        self.names = [n.decode() for n in names]
        self.descs = [d.decode() for d in descs]
        self.lengths = np.array([len(p) for p in parts], dtype=np.int64)
        off = np.zeros(self.nseq + 1, dtype=np.uint64)
        np.cumsum(self.lengths, out=off[1:])
        text = b"".join(parts)
        self.bin_off = np.array(bin_off, dtype=np.uint32)
        na = (C.c_char_p * max(1, self.nseq))(*names)
        da = (C.c_char_p * max(1, self.nseq))(*descs)
        self.h = C.c_void_p()
        _chk(load().ckm_seqs_pack(ctx.h, text, off.ctypes.data, self.nseq, self.bin_off.ctypes.data, self.nbins, na, da,
                                  C.byref(self.h)))
        self.total_residues = int(self.lengths.sum())

    def close(self):
        if self.h:
            load().ckm_seqs_free(self.h)
            self.h = C.c_void_p()


class Hits(object):
    def __init__(self, h):
        self.h = h
        cols = HitColumns()
        _chk(load().ckm_hits_columns(h, C.byref(cols)))
        self.cols = cols
        self.n = int(cols.n)
        self.nbins = int(cols.nbins)
        self.bin_row_off = np.ctypeslib.as_array(cols.bin_row_off, shape=(self.nbins + 1,)).copy()
        for f in HIT_FIELDS:
            ptr = getattr(cols, f)
            setattr(self, f, np.ctypeslib.as_array(ptr, shape=(self.n,)).copy() if self.n else np.zeros(0))

    def rows(self, b):
        return range(int(self.bin_row_off[b]), int(self.bin_row_off[b + 1]))

    def write_domtblout(self, profiles, seqs, b, path):
        _chk(load().ckm_hits_write_domtblout(self.h, profiles.h, seqs.h, b, path.encode()))

    def write_alignments(self, ctx, profiles, seqs, b, path):
        """hmmsearch-style report of bin b with the domain alignments (what `-o` holds when CheckM keeps alignments)."""
        _chk(load().ckm_hits_write_alignments(ctx.h, self.h, profiles.h, seqs.h, b, path.encode()))

    def close(self):
        if self.h:
            load().ckm_hits_free(self.h)
            self.h = None


class Tables(object):
    """domtblout text of many bins, parsed by the library (ckm_tables_read); column views + the ext form ckm_reduce takes."""

    def __init__(self, paths):
        arr = (C.c_char_p * max(1, len(paths)))(*[p.encode() for p in paths])
        h = C.c_void_p()
        _chk(load().ckm_tables_read(arr, len(paths), C.byref(h)))
        self.h = h
        self._refresh()

    def _refresh(self):
        tc = TableColumns()
        _chk(load().ckm_tables_get(self.h, C.byref(tc)))
        self.tc = tc
        cols = tc.cols
        self.n = int(cols.n)
        self.nbins = int(cols.nbins)
        self.bin_row_off = np.ctypeslib.as_array(cols.bin_row_off, shape=(self.nbins + 1,)).copy()
        self.missing = np.ctypeslib.as_array(tc.bin_missing, shape=(max(1, self.nbins),)).copy()[:self.nbins].astype(bool)

    def assign_models(self, keys):
        """keys: markerHits key of every model slot; returns the number of rows whose accession is not among them."""
        arr = (C.c_char_p * max(1, len(keys)))(*[k.encode() for k in keys])
        miss = C.c_uint64()
        _chk(load().ckm_tables_assign_models(self.h, arr, len(keys), C.byref(miss)))
        self._refresh()
        return int(miss.value)

    def column(self, name):
        ptr = getattr(self.tc, name) if name in ("full_bias_d", "dom_bias_d", "acc_d") else getattr(self.tc.cols, name)
        return np.ctypeslib.as_array(ptr, shape=(self.n,)) if self.n else np.zeros(0)

    def hit(self, r):
        """Row r as the reference's HmmerHitDOM would hold it (checkm/hmmer.py:255-285): Python ints, floats and strings."""
        c, t = self.tc.cols, self.tc
        return dict(target_name=c.target_name[r].decode(), target_accession=t.target_accession[r].decode(), target_length=int(c.tlen[r]),
                    query_name=t.query_name[r].decode(), query_accession=t.query_accession[r].decode(), query_length=int(c.qlen[r]),
                    full_e_value=float(c.full_evalue[r]), full_score=float(c.full_score_d[r]), full_bias=float(t.full_bias_d[r]),
                    dom=int(c.dom_idx[r]), ndom=int(c.ndom[r]), c_evalue=float(c.c_evalue[r]), i_evalue=float(c.i_evalue[r]),
                    dom_score=float(c.dom_score_d[r]), dom_bias=float(t.dom_bias_d[r]), hmm_from=int(c.hmm_from[r]), hmm_to=int(c.hmm_to[r]),
                    ali_from=int(c.ali_from[r]), ali_to=int(c.ali_to[r]), env_from=int(c.env_from[r]), env_to=int(c.env_to[r]),
                    acc=float(t.acc_d[r]), target_description=t.description[r].decode())

    def text(self, name, r):
        v = getattr(self.tc, name)[r] if name != "target_name" else self.tc.cols.target_name[r]
        return v.decode()

    def ext(self):
        """(HitColumns, keepalive) for QAPlan.reduce(ext=...)."""
        return self.tc.cols, [self]

    def close(self):
        if self.h:
            load().ckm_tables_free(self.h)
            self.h = None


def search(ctx, profiles, seqs, bin_models=None, E=0.1, domE=0.1):
    """bin_models: None (all models for every bin) or a list (per bin) of model-index lists."""
    out = C.c_void_p()
    if bin_models is None:
        _chk(load().ckm_search(ctx.h, profiles.h, seqs.h, None, None, E, domE, C.byref(out)))
    else:
        off = np.zeros(len(bin_models) + 1, dtype=np.uint32)
        for i, m in enumerate(bin_models):
            off[i + 1] = off[i] + len(m)
        flat = [x for m in bin_models for x in m]
        idx = np.array(flat if flat else [0], dtype=np.uint32)
        _chk(load().ckm_search(ctx.h, profiles.h, seqs.h, off.ctypes.data, idx.ctypes.data, E, domE, C.byref(out)))
    return Hits(out)


def debug_stages(ctx, profiles, seqs, model, seq):
    model = np.ascontiguousarray(model, dtype=np.uint32)
    seq = np.ascontiguousarray(seq, dtype=np.uint32)
    out = (StageScores * len(model))()
    _chk(load().ckm_debug_stages(ctx.h, profiles.h, seqs.h, model.ctypes.data, seq.ctypes.data, len(model), out))
    return out


def debug_ssv(ctx, profiles, seqs, model, seq, per_block=0, lanes=0):
    """The SSV kernel as the search launches it, one model against `seq` in the given order: (Smax uint16[n], route uint8[n] -- 0 dropped,
    1 survivor, 2 exact MSV kernel --, usc float32[n] of the survivors, {cls, threads, per_block, nblocks})."""
    seq = np.ascontiguousarray(seq, dtype=np.uint32)
    smax = np.zeros(len(seq), dtype=np.uint16)
    route = np.zeros(len(seq), dtype=np.uint8)
    usc = np.zeros(len(seq), dtype=np.float32)
    info = np.zeros(4, dtype=np.int32)
    _chk(load().ckm_debug_ssv(ctx.h, profiles.h, seqs.h, int(model), seq.ctypes.data, len(seq), int(per_block), int(lanes), smax.ctypes.data,
                              route.ctypes.data, usc.ctypes.data, info.ctypes.data))
    return smax, route, usc, dict(cls=int(info[0]), threads=int(info[1]), per_block=int(info[2]), nblocks=int(info[3]))


FILTERS_VIT16, FILTERS_WAVE_FAST, FILTERS_WAVE_FAST_PLAIN, FILTERS_CHAIN = 0, 1, 2, 3
FILTER_RESULT = np.dtype([("bias_d", "<f4"), ("bias_e", "<f4"), ("filtersc", "<f4"), ("vit_fast", "<f4"), ("vit_exact", "<f4"), ("vit_xC", "<i4"),
                          ("vit_flag", "<u4"), ("route", "<u4"), ("n_vq", "<u4"), ("n_vxq", "<u4"), ("n_fwork", "<u4")])


def debug_filters(ctx, profiles, seqs, model, seq, usc, filtersc, mode, nblocks=0):
    """The bias filter and the Viterbi kernels as the device-driven search runs them on the pairs (model[i], seq[i]) in the given order
    (include/checkm_hip.h: ckm_debug_filters): (a FILTER_RESULT record array, the cascade's status word)."""
    model = np.ascontiguousarray(model, dtype=np.uint32)
    seq = np.ascontiguousarray(seq, dtype=np.uint32)
    usc = np.ascontiguousarray(usc, dtype=np.float32)
    fsc = None if filtersc is None else np.ascontiguousarray(filtersc, dtype=np.float32)
    assert len(seq) == len(model) == len(usc) and (fsc is None or len(fsc) == len(model))
    out = np.zeros(len(model), dtype=FILTER_RESULT)
    status = C.c_uint32(0)
    _chk(load().ckm_debug_filters(ctx.h, profiles.h, seqs.h, model.ctypes.data, seq.ctypes.data, usc.ctypes.data,
                                  None if fsc is None else fsc.ctypes.data, len(model), int(mode), int(nblocks), out.ctypes.data, C.byref(status)))
    return out, int(status.value)


def debug_envelopes(ctx, profiles, seqs, model, seq, ienv, jenv):
    model = np.ascontiguousarray(model, dtype=np.uint32)
    seq = np.ascontiguousarray(seq, dtype=np.uint32)
    ienv = np.ascontiguousarray(ienv, dtype=np.int32)
    jenv = np.ascontiguousarray(jenv, dtype=np.int32)
    out = (EnvelopeResult * len(model))()
    _chk(load().ckm_debug_envelopes(ctx.h, profiles.h, seqs.h, model.ctypes.data, seq.ctypes.data, ienv.ctypes.data,
                                    jenv.ctypes.data, len(model), out))
    return out


def debug_envelope_paths(ctx, profiles, seqs, model, seq, ienv, jenv):
    """The optimal-accuracy paths of chosen envelopes with their posterior lines: (ok[n], [int32[M] per envelope: the envelope-local
    residue of every match node, 0 = none], [float32[Ld + 1] per envelope: the posterior of every residue on the path])."""
    model = np.ascontiguousarray(model, dtype=np.uint32)
    seq = np.ascontiguousarray(seq, dtype=np.uint32)
    ienv = np.ascontiguousarray(ienv, dtype=np.int32)
    jenv = np.ascontiguousarray(jenv, dtype=np.int32)
    n = len(model)
    off, ppo = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([profiles.headers[int(m)]["leng"] for m in model], dtype=np.uint64)
    ppo[1:] = np.cumsum(jenv.astype(np.int64) - ienv + 2, dtype=np.uint64)
    ok = np.zeros(max(1, n), dtype=np.int32)
    path, pp = np.zeros(max(1, int(off[-1])), dtype=np.int32), np.zeros(max(1, int(ppo[-1])), dtype=np.float32)
    _chk(load().ckm_debug_envelope_paths(ctx.h, profiles.h, seqs.h, model.ctypes.data, seq.ctypes.data, ienv.ctypes.data, jenv.ctypes.data, n,
                                         ok.ctypes.data, off.ctypes.data, path.ctypes.data, ppo.ctypes.data, pp.ctypes.data))
    return ok[:n], [path[int(off[j]):int(off[j + 1])].copy() for j in range(n)], [pp[int(ppo[j]):int(ppo[j + 1])].copy() for j in range(n)]


def debug_region(ctx, profiles, seqs, model, seq, ireg, jreg, cap=64):
    """Trace ensemble of one region: (n2sum[Lr], segs[200][cap][4], nseg[200], envelopes[n][4]), region-local coordinates."""
    n2 = np.zeros(jreg - ireg + 1, dtype=np.float32)
    segs = np.zeros((200, cap, 4), dtype=np.int32)
    nseg = np.zeros(200, dtype=np.int32)
    env = np.zeros((64, 4), dtype=np.int32)
    nenv = C.c_int32()
    _chk(load().ckm_debug_region(ctx.h, profiles.h, seqs.h, model, seq, ireg, jreg, n2.ctypes.data, segs.ctypes.data, nseg.ctypes.data, cap,
                                 env.ctypes.data, 64, C.byref(nenv)))
    return n2, segs, nseg, env[:nenv.value].copy()


def align(ctx, profiles, seqs, model, seq):
    """Optimal-accuracy alignment of whole sequences to models (what hmmalign computes per sequence): list of int32 arrays, one per
    pair, of length M: 1-based residue emitted by each match state, 0 = none."""
    model = np.ascontiguousarray(model, dtype=np.uint32)
    seq = np.ascontiguousarray(seq, dtype=np.uint32)
    off = np.zeros(len(model) + 1, dtype=np.uint64)
    for j, m in enumerate(model):
        off[j + 1] = off[j] + profiles.headers[int(m)]["leng"]
    out = np.zeros(max(1, int(off[-1])), dtype=np.int32)
    _chk(load().ckm_align(ctx.h, profiles.h, seqs.h, model.ctypes.data, seq.ctypes.data, len(model), off.ctypes.data, out.ctypes.data))
    return [out[int(off[j]):int(off[j + 1])].copy() for j in range(len(model))]


def orf_nodes(ctx, contigs, trans_table=11, closed=False):
    """Start / stop nodes of all six frames of a bin's contigs (ckm_orf_scan): contigs = list of nucleotide strings (or bytes).
    Returns (columns dict of numpy arrays: contig, ndx, stop_val, type, strand_rev, edge; stats dict)."""
    parts = [c.encode() if isinstance(c, str) else bytes(c) for c in contigs]
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    np.cumsum([len(p) for p in parts], out=off[1:])
    text = b"".join(parts)
    h = C.c_void_p()
    _chk(load().ckm_orf_scan(ctx.h, text, off.ctypes.data, len(parts), int(trans_table), 1 if closed else 0, C.byref(h)))
    try:
        cols = OrfColumns()
        _chk(load().ckm_orf_columns_get(h, C.byref(cols)))
        n = int(cols.n)
        arr = np.ctypeslib.as_array
        out = {f: (arr(getattr(cols, f), shape=(n,)).copy() if n else np.zeros(0, dtype=np.int64)) for f in ("contig", "ndx", "stop_val", "type", "strand_rev", "edge")}
        stats = dict(ms_flags=cols.ms_flags, ms_chain=cols.ms_chain, bases=int(cols.bases), padded_bytes=int(cols.padded_bytes))
    finally:
        load().ckm_orf_free(h)
    return out, stats


GENE_FIELDS = ("bin", "contig", "begin", "end", "strand", "start_type", "partial_left", "partial_right", "rbs_bin", "mot_len", "mot_ndx", "mot_spacer",
               "gc_cont", "conf", "score", "cscore", "sscore", "rscore", "uscore", "tscore")


class GeneBatch(object):
    """The nucleotides of a batch of bins laid out for ckm_genes_call: bins = [[(contig id, sequence as str or bytes), ...], ...]
    (or plain sequences).  One batch serves both translation tables and the writers."""

    def __init__(self, bins):
        parts, ids, bin_first = [], [], [0]
        for contigs in bins:
            for c in contigs:
                cid, seq = c if isinstance(c, tuple) else ("", c)
                parts.append(seq.encode() if isinstance(seq, str) else bytes(seq))
                ids.append(cid.encode() if isinstance(cid, str) else bytes(cid))
            bin_first.append(len(parts))
        self.nbins, self.ncontigs = len(bins), len(parts)
        self.off = np.zeros(len(parts) + 1, dtype=np.uint64)
        if parts:
            np.cumsum([len(p) for p in parts], out=self.off[1:])
        self.bin_first = np.asarray(bin_first, dtype=np.uint32)
        self.text = b"".join(parts)
        self.ids = (C.c_char_p * max(1, len(ids)))(*ids)
        self.bases = [int(self.off[bin_first[b + 1]] - self.off[bin_first[b]]) for b in range(self.nbins)]
        self._h = None

    @classmethod
    def from_files(cls, paths):
        """The batch of the plain nucleotide FASTA files `paths`, a bin each, read and laid out by the library's host threads
        (ckm_nuc_batch_read: the record rules of geneFinder.read_contigs_bytes) -- no Python object per contig, no interpreter lock held."""
        self = cls.__new__(cls)
        arr = (C.c_char_p * max(1, len(paths)))(*[p.encode() for p in paths])
        h = C.c_void_p()
        _chk(load().ckm_nuc_batch_read(arr, len(paths), C.byref(h)))
        self._h = h
        v = NucBatchView()
        _chk(load().ckm_nuc_batch_view_get(h, C.byref(v)))
        self.nbins, self.ncontigs = int(v.nbins), int(v.ncontigs)
        self.off = np.ctypeslib.as_array(v.contig_off, shape=(self.ncontigs + 1,))
        total = int(self.off[-1])
        # views of the library's batch (alive until close): the text as bytes-like uint8, the ids as an address
        self.text = np.ctypeslib.as_array((C.c_uint8 * total).from_address(v.text)) if total else np.zeros(0, dtype=np.uint8)
        self.ids = v.contig_ids
        self.bin_first = np.ctypeslib.as_array(v.bin_first, shape=(self.nbins + 1,))
        self.bases = [int(x) for x in np.ctypeslib.as_array(v.bin_bases, shape=(self.nbins,))] if self.nbins else []
        return self

    def text_arg(self):
        """The text as ckm_genes_call / ckm_genes_write_bin take it."""
        return self.text if isinstance(self.text, bytes) else self.text.ctypes.data

    def contigs(self, b):
        """[(id bytes, sequence bytes)] of bin b (tests, diagnostics)."""
        out = []
        for c in range(int(self.bin_first[b]), int(self.bin_first[b + 1])):
            a, z = int(self.off[c]), int(self.off[c + 1])
            if self._h is None:
                out.append((self.ids[c], self.text[a:z]))
            else:
                out.append((C.cast(self.ids + c * C.sizeof(C.c_void_p), C.POINTER(C.c_char_p))[0], self.text[a:z].tobytes()))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self.off = self.bin_first = self.text = None
            load().ckm_nuc_batch_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GeneCall(object):
    """Result of one ckm_genes_call (a batch of bins, one translation table); close() frees it."""

    def __init__(self, ctx, batch, trans_table=11, closed=False, mask=True):
        self.batch, self.table = batch, int(trans_table)
        self.h = C.c_void_p()
        _chk(load().ckm_genes_call(ctx.h, batch.text_arg(), batch.off.ctypes.data, batch.ncontigs, batch.bin_first.ctypes.data, batch.nbins, self.table, 1 if closed else 0, 1 if mask else 0, C.byref(self.h)))
        cols = GeneColumns()
        _chk(load().ckm_genes_columns_get(self.h, C.byref(cols)))
        self._cols = cols
        nb = int(cols.nbins)
        arr = np.ctypeslib.as_array
        self.per_bin = {f: (arr(getattr(cols, "bin_" + f), shape=(nb,)).copy() if nb else np.zeros(0)) for f in ("trained", "uses_sd", "gc", "bases", "coding", "nodes")}
        self.stats = dict(ms_nodes=cols.ms_nodes, ms_dp_train=cols.ms_dp_train, ms_score=cols.ms_score, ms_dp_find=cols.ms_dp_find, ms_total=cols.ms_total)
        self.ngenes = int(cols.n)

    def columns(self):
        """Columns dict of numpy arrays over all genes + 'proteins' list of str; `contig` is the contig's index inside its bin."""
        cols, n = self._cols, self.ngenes
        arr = np.ctypeslib.as_array
        out = {f: (arr(getattr(cols, f), shape=(n,)).copy() if n else np.zeros(0, dtype=np.int64)) for f in GENE_FIELDS}
        if n:
            out["contig"] = out["contig"] - self.batch.bin_first[out["bin"]]
        po = arr(cols.prot_off, shape=(n + 1,)).copy() if n else np.zeros(1, dtype=np.uint64)
        blob = C.string_at(cols.prot, int(po[-1])) if n else b""
        txt, pl = blob.decode("ascii"), po.tolist()
        out["proteins"] = [txt[a:b] for a, b in zip(pl[:-1], pl[1:])]
        return out

    def genes_per_bin(self):
        if not self.ngenes:
            return np.zeros(self.batch.nbins, dtype=np.int64)
        b = np.ctypeslib.as_array(self._cols.bin, shape=(self.ngenes,))
        return np.bincount(b, minlength=self.batch.nbins)

    def coding_union(self):
        """Bases of every bin covered by at least one gene (checkm/prodigal.py:246-274)."""
        out = np.zeros(max(1, self.batch.nbins), dtype=np.uint64)
        _chk(load().ckm_genes_coding_union(self.h, out.ctypes.data))
        return out[:self.batch.nbins]

    def write_bin(self, b, aaFile, gffFile, ntFile=None):
        bt = self.batch
        _chk(load().ckm_genes_write_bin(self.h, int(b), self.table, bt.ids, bt.text_arg(), bt.off.ctypes.data, bt.bin_first.ctypes.data,
                                        aaFile.encode(), gffFile.encode(), ntFile.encode() if ntFile else None))

    def close(self):
        if self.h:
            load().ckm_genes_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def call_genes(ctx, bins, trans_table=11, closed=False, mask=True):
    """Gene calling for a batch of bins (ckm_genes_call): bins = list of lists of nucleotide strings / bytes (the contigs of each bin).
    Returns (columns dict of numpy arrays over all genes + 'proteins' list of str, per-bin dict, stats dict); `contig` is the contig's
    index inside its bin."""
    call = GeneCall(ctx, GeneBatch(bins), trans_table, closed, mask)
    try:
        return call.columns(), call.per_bin, call.stats
    finally:
        call.close()


def debug_orf_flags(ctx, nbytes, reps=10):
    """Average duration (ms) of one launch of the streaming codon-flag kernel over nbytes of device-generated nucleotides."""
    ms = C.c_double()
    _chk(load().ckm_debug_orf_flags(ctx.h, int(nbytes), int(reps), C.byref(ms)))
    return ms.value


class NucSeqs(object):
    """Nucleotide FASTA files read with the rules of CheckM's readFasta (ckm_nucseq_read, checkm/util/seqUtils.py:180-211), on the
    library's host threads; the batch stays in the library until close()."""

    def __init__(self, paths):
        arr = (C.c_char_p * max(1, len(paths)))(*[os.fsencode(p) for p in paths])
        self.h = C.c_void_p()
        _chk(load().ckm_nucseq_read(arr, len(paths), C.byref(self.h)))
        v = NucSeqView()
        _chk(load().ckm_nucseq_view_get(self.h, C.byref(v)))
        self.nseq, self.nfiles = int(v.nseq), int(v.nfiles)
        arr = np.ctypeslib.as_array
        self.seq_off = arr(v.seq_off, shape=(self.nseq,)).copy() if self.nseq else np.zeros(0, dtype=np.uint64)
        self.seq_bytes = arr(v.seq_bytes, shape=(self.nseq,)).copy() if self.nseq else np.zeros(0, dtype=np.uint64)
        self.file_first = arr(v.file_first, shape=(self.nfiles + 1,)).copy()
        self._view = v

    def ids(self, f=None):
        """Sequence ids (str) of file f, or of the whole batch, in the reference's dict order."""
        a, z = (0, self.nseq) if f is None else (int(self.file_first[f]), int(self.file_first[f + 1]))
        return [self._view.seq_ids[i].decode("utf-8") for i in range(a, z)]

    def seq(self, i):
        """Sequence i as bytes (UTF-8)."""
        return C.string_at(self._view.text + int(self.seq_off[i]), int(self.seq_bytes[i]))

    def close(self):
        if self.h:
            load().ckm_nucseq_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def nucstats(ctx, seqs, tetra=False, tile_bytes=0):
    """The device pass over a NucSeqs batch (ckm_nucstats_run).  Returns a dict: count [nseq, 8] uint64 (A, C, G, T+U, N, n, code
    points, code points other than N), piece_off [nseq + 1], piece_len, tetra [nseq, 136] uint32 or None, and the timings."""
    h = C.c_void_p()
    _chk(load().ckm_nucstats_run(ctx.h, seqs.h, 1 if tetra else 0, int(tile_bytes), C.byref(h)))
    try:
        c = NucStatsColumns()
        _chk(load().ckm_nucstats_columns_get(h, C.byref(c)))
        n = int(c.nseq)
        arr = np.ctypeslib.as_array
        npieces = int(c.piece_off[n]) if n else 0
        out = dict(count=arr(c.count, shape=(n, 8)).copy() if n else np.zeros((0, 8), dtype=np.uint64),
                   piece_off=arr(c.piece_off, shape=(n + 1,)).copy(),
                   piece_len=arr(c.piece_len, shape=(npieces,)).copy() if npieces else np.zeros(0, dtype=np.uint64),
                   tetra=(arr(c.tetra, shape=(n, 136)).copy() if n else np.zeros((0, 136), dtype=np.uint32)) if tetra else None,
                   bytes=int(c.bytes), tiles=int(c.tiles), run_starts=int(c.run_starts),
                   ms_upload=c.ms_upload, ms_count=c.ms_count, ms_fill=c.ms_fill, ms_total=c.ms_total)
    finally:
        load().ckm_nucstats_free(h)
    return out


def bin_genes(seqs, gff_paths, faa_paths):
    """(coding bases, translation table or None, gene count) per file of the batch, (-1, -1, -1) without a GFF (ckm_bin_genes_read)."""
    n = seqs.nfiles
    g = (C.c_char_p * max(1, n))(*[os.fsencode(p) for p in gff_paths])
    a = (C.c_char_p * max(1, n))(*[os.fsencode(p) for p in faa_paths])
    coding, ngenes = np.zeros(max(1, n), dtype=np.int64), np.zeros(max(1, n), dtype=np.int64)
    table = np.zeros(max(1, n), dtype=np.int32)
    _chk(load().ckm_bin_genes_read(g, a, seqs.h, coding.ctypes.data, table.ctypes.data, ngenes.ctypes.data))
    return [(int(coding[k]), None if table[k] == -2 ** 31 else int(table[k]), int(ngenes[k])) for k in range(n)]


def seq_genes(seqs, gff_paths):
    """(coding bases per sequence of the batch [nseq] int64, missing [nfiles] bool) from bins/<binId>/genes.gff of every file
    (ckm_seq_genes_read): ProdigalGeneFeatureParser.codingBases(seqId), -1 for the sequences of a file without a GFF."""
    n = seqs.nfiles
    g = (C.c_char_p * max(1, n))(*[os.fsencode(p) for p in gff_paths])
    coding = np.zeros(max(1, seqs.nseq), dtype=np.int64)
    missing = np.zeros(max(1, n), dtype=np.uint8)
    _chk(load().ckm_seq_genes_read(g, seqs.h, coding.ctypes.data, missing.ctypes.data))
    return coding[:seqs.nseq], missing[:n].astype(bool)


class TetraProfile(object):
    """The file GenomicSignatures.calculate writes, parsed once by the library's host threads (ckm_tetra_profile_read); every value is
    float(token) bit for bit.  Lives in the library until close()."""

    def __init__(self, path):
        self.h = C.c_void_p()
        _chk(load().ckm_tetra_profile_read(os.fsencode(path), C.byref(self.h)))
        v = TetraProfileView()
        _chk(load().ckm_tetra_profile_view_get(self.h, C.byref(v)))
        self.n = int(v.n)
        self._view = v

    def ids(self):
        return [self._view.ids[i].decode("utf-8") for i in range(self.n)]

    def sig(self):
        """[n, 136] float64 (a copy)."""
        return np.ctypeslib.as_array(self._view.sig, shape=(self.n, 136)).copy() if self.n else np.zeros((0, 136))

    def gather(self, seqs):
        """([nseq, 136] rows of the batch's sequences by id, index of the first sequence the profile does not hold or -1)."""
        out = np.zeros((max(1, seqs.nseq), 136), dtype=np.float64)
        miss = C.c_int64(-1)
        _chk(load().ckm_tetra_profile_gather(self.h, seqs.h, out.ctypes.data, C.byref(miss)))
        return out[:seqs.nseq], int(miss.value)

    def close(self):
        if self.h:
            load().ckm_tetra_profile_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def outliers(ctx, seqs, count, sig, coding, tab_off, key, lo, hi, bin_gc_tab, bin_cd_tab, td_tab):
    """The device pass of `checkm outliers` over a NucSeqs batch (ckm_outliers_run): count = nucstats()['count'], sig = the gathered
    profile rows, coding = seq_genes()[0]; the bound tables as include/checkm_hip.h lays them out.  Returns a dict of per-sequence
    float64 columns gc, delta_gc, cd, delta_cd, td, weight, the flag bytes (bit 0 GC, 1 CD, 2 TD), per-bin mean_gc, mean_cd,
    bin_sig [nbins, 136] and the timings.  Raises ZeroDivisionError where the reference does (a sequence without A, C, G, T, U)."""
    count = np.ascontiguousarray(count, dtype=np.uint64)
    sig = np.ascontiguousarray(sig, dtype=np.float64)
    coding = np.ascontiguousarray(coding, dtype=np.int64)
    assert count.shape == (seqs.nseq, 8) and sig.shape == (seqs.nseq, 136) and coding.shape == (seqs.nseq,)
    tab_off = np.ascontiguousarray(tab_off, dtype=np.uint32)
    key, lo, hi = (np.ascontiguousarray(x, dtype=np.float64) for x in (key, lo, hi))
    assert len(key) == len(lo) == len(hi) == int(tab_off[-1])
    gct, cdt = (np.ascontiguousarray(x, dtype=np.uint32) for x in (bin_gc_tab, bin_cd_tab))
    assert len(gct) == len(cdt) == seqs.nfiles
    keep = [np.zeros(1, dtype=x.dtype) if x.size == 0 else x for x in (count, sig, coding, gct, cdt)]
    b = OutlierBounds(len(tab_off) - 1, tab_off.ctypes.data, key.ctypes.data, lo.ctypes.data, hi.ctypes.data, keep[3].ctypes.data, keep[4].ctypes.data, int(td_tab))
    h = C.c_void_p()
    zero = C.c_int64(-1)
    rc = load().ckm_outliers_run(ctx.h, seqs.h, keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, C.byref(b), C.byref(zero), C.byref(h))
    if rc != 0 and zero.value >= 0:
        raise ZeroDivisionError("float division by zero")
    _chk(rc)
    try:
        c = OutlierColumns()
        _chk(load().ckm_outliers_columns_get(h, C.byref(c)))
        n, nb = int(c.nseq), int(c.nbins)
        arr = np.ctypeslib.as_array
        out = {f: (arr(getattr(c, f), shape=(n,)).copy() if n else np.zeros(0)) for f in ("gc", "delta_gc", "cd", "delta_cd", "td", "weight")}
        out["flags"] = arr(c.flags, shape=(n,)).copy() if n else np.zeros(0, dtype=np.uint8)
        out["mean_gc"] = arr(c.mean_gc, shape=(nb,)).copy() if nb else np.zeros(0)
        out["mean_cd"] = arr(c.mean_cd, shape=(nb,)).copy() if nb else np.zeros(0)
        out["bin_sig"] = arr(c.bin_sig, shape=(nb, 136)).copy() if nb else np.zeros((0, 136))
        for f in ("ms_upload", "ms_seq", "ms_binsig", "ms_td", "ms_flags", "ms_total"):
            out[f] = getattr(c, f)
    finally:
        load().ckm_outliers_free(h)
    return out


MERGE_COLUMNS = ("comp_i", "cont_i", "comp_j", "cont_j", "delta_comp", "delta_cont", "delta", "comp_merged", "cont_merged")


def _merge_args(member_bits, hit_sum, n_markers, ngenes, thresholds):
    bits = np.ascontiguousarray(member_bits, dtype=np.uint64)
    nwords = (int(ngenes) + 63) // 64
    if bits.ndim != 2 or bits.shape[1] != max(1, nwords):
        raise ValueError("member_bits must be [nbins, (ngenes + 63) // 64]")
    s = np.ascontiguousarray(hit_sum, dtype=np.int64)
    n = np.ascontiguousarray(n_markers, dtype=np.int32)
    if s.shape != (bits.shape[0],) or n.shape != (bits.shape[0],):
        raise ValueError("hit_sum and n_markers must hold one value per bin")
    thr = np.ascontiguousarray([float(x) for x in thresholds], dtype=np.float64)
    if thr.shape != (4,):
        raise ValueError("four thresholds")
    return bits, s, n, thr


def merge_check(member_bits, hit_sum, n_markers, ngenes, thresholds):
    """ckm_merge_check: the argument tests of merge_pairs(), without a device.  Raises CkmError as merge_pairs would."""
    bits, s, n, thr = _merge_args(member_bits, hit_sum, n_markers, ngenes, thresholds)
    _chk(load().ckm_merge_check(bits.shape[0], int(ngenes), bits.ctypes.data, s.ctypes.data, n.ctypes.data, thr.ctypes.data))


def merge_pairs(ctx, member_bits, hit_sum, n_markers, ngenes, thresholds, bin_ids=None, append_path=None, budget_bytes=0, keep_columns=True):
    """The all-pairs comparison of `checkm merge` (ckm_merge_run): member_bits [nbins, nwords] uint64, one row per bin in output order;
    thresholds = (minDeltaComp, maxDeltaCont, minMergedComp, maxMergedCont).  append_path: the lines of the reported pairs are appended
    to that file (bin_ids: the encoded ids).  Returns a dict: npairs, compared, nbatches, the timings and, with keep_columns, i, j and
    the nine float64 columns of MERGE_COLUMNS."""
    bits, s, n, thr = _merge_args(member_bits, hit_sum, n_markers, ngenes, thresholds)
    nb = bits.shape[0]
    ids = None
    if bin_ids is not None:
        if len(bin_ids) != nb:
            raise ValueError("one id per bin")
        ids = (C.c_char_p * max(1, nb))(*[b if isinstance(b, bytes) else b.encode() for b in bin_ids])
    h = C.c_void_p()
    _chk(load().ckm_merge_run(ctx.h, nb, int(ngenes), bits.ctypes.data, s.ctypes.data, n.ctypes.data, thr.ctypes.data, ids,
                              os.fsencode(append_path) if append_path is not None else None, int(budget_bytes), 1 if keep_columns else 0, C.byref(h)))
    try:
        c = MergeColumns()
        _chk(load().ckm_merge_columns_get(h, C.byref(c)))
        out = dict(npairs=int(c.npairs), compared=int(c.compared), nbatches=int(c.nbatches))
        for f in ("ms_upload", "ms_bins", "ms_count", "ms_scan", "ms_fill", "ms_download", "ms_write", "ms_total"):
            out[f] = getattr(c, f)
        if c.kept:
            k = out["npairs"]
            arr = np.ctypeslib.as_array
            out["i"] = arr(c.i, shape=(k,)).copy() if k else np.zeros(0, dtype=np.uint32)
            out["j"] = arr(c.j, shape=(k,)).copy() if k else np.zeros(0, dtype=np.uint32)
            for q, f in enumerate(MERGE_COLUMNS):
                out[f] = arr(c.col[q], shape=(k,)).copy() if k else np.zeros(0)
    finally:
        load().ckm_merge_free(h)
    return out


COVERAGE_SLOTS = ("reads", "duplicates", "secondary", "failed_qc", "failed_align_len", "failed_edit_dist", "failed_proper_pair", "mapped", "numerator")
COVERAGE_REASONS = {1: "an auxiliary field runs past the record", 2: "tag 'NM' not present", 3: "tag 'NM' is not an integer", 4: "an auxiliary field of unknown type",
                    5: "the read has no CIGAR", 6: "a mapped read starts before its reference"}          # (5 and 6: coverage_windows only)
COVWIN_SCAN_BLOCK = 1024          # slots per workgroup of the scan over the windows (covwin_dev.h: SCAN_BLOCK)


class CoverageRecordError(CkmError):
    """A record the device pass could not classify: reason (COVERAGE_REASONS), record (ordinal in the file), read (its name)."""

    def __init__(self, code, msg, reason, record, read):
        CkmError.__init__(self, code, msg)
        self.reason, self.record, self.read = reason, record, read


class Bam(object):
    """A BAM file opened by the library's host reader (ckm_bam_open: BGZF blocks, header; no device, no index).  Read once."""

    def __init__(self, path):
        self.path = path
        self.h = C.c_void_p()
        _chk(load().ckm_bam_open(os.fsencode(path), C.byref(self.h)))
        v = BamHeaderView()
        _chk(load().ckm_bam_header(self.h, C.byref(v)))
        n = int(v.n_ref)
        self.references = [v.names[k].decode("utf-8") for k in range(n)]
        self.lengths = [int(v.lengths[k]) for k in range(n)]
        self.header_bytes = int(v.header_bytes)

    def close(self):
        if self.h:
            load().ckm_bam_close(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _coverage_params(all_reads, min_align_per, max_edit_dist_per, min_qc, budget_bytes):
    return CoverageParams(float(min_align_per), float(max_edit_dist_per), float(min_qc), 1 if all_reads else 0, int(budget_bytes))


def coverage_check(all_reads, min_align_per, max_edit_dist_per, min_qc):
    """ckm_coverage_check: the parameter tests of coverage_counters(), without a device."""
    p = _coverage_params(all_reads, min_align_per, max_edit_dist_per, min_qc, 0)
    _chk(load().ckm_coverage_check(C.byref(p)))


def coverage_counters(ctx, bam, all_reads, min_align_per, max_edit_dist_per, min_qc, budget_bytes=0):
    """The device pass over every record of an open Bam (ckm_coverage_run): ([n_ref, 9] int64 in the order of COVERAGE_SLOTS, timing
    dict).  Raises CoverageRecordError for a record whose auxiliary fields cannot be walked or whose NM is needed and missing."""
    p = _coverage_params(all_reads, min_align_per, max_edit_dist_per, min_qc, budget_bytes)
    out = np.zeros((max(1, len(bam.references)), len(COVERAGE_SLOTS)), dtype=np.int64)
    t = CoverageTiming()
    rc = load().ckm_coverage_run(ctx.h, bam.h, C.byref(p), out.ctypes.data, C.byref(t))
    if rc != 0 and t.error_reason:
        raise CoverageRecordError(rc, load().ckm_last_error().decode(errors="replace"), int(t.error_reason), int(t.error_record), t.error_read.decode(errors="replace"))
    _chk(rc)
    timing = {f: getattr(t, f) for f in ("records", "batches", "blocks", "inflated_bytes", "ms_read", "ms_inflate", "ms_offsets", "ms_upload", "ms_kernel", "ms_download", "ms_total")}
    return out[:len(bam.references)], timing


def _coverage_windows_params(all_reads, min_align_per, max_edit_dist_per, window_size, budget_bytes):
    w = int(window_size)
    return CoverageWindowsParams(float(min_align_per), float(max_edit_dist_per), 1 if all_reads else 0, max(-1, min(w, 1 << 62)), int(budget_bytes))


def coverage_windows_check(all_reads, min_align_per, max_edit_dist_per, window_size):
    """ckm_coverage_windows_check: the parameter tests of coverage_windows(), without a device."""
    p = _coverage_windows_params(all_reads, min_align_per, max_edit_dist_per, window_size, 0)
    _chk(load().ckm_coverage_windows_check(C.byref(p)))


def coverage_windows_layout(bam, window_size):
    """ckm_coverage_windows_layout: [n_ref + 1] int64, the first slot of every reference and the number of slots; reference k has
    (L - 1) // w + 1 slots for L > 0 -- its reported windows and the tail."""
    first = np.zeros(len(bam.references) + 1, dtype=np.int64)
    _chk(load().ckm_coverage_windows_layout(bam.h, max(-1, min(int(window_size), 1 << 62)), first.ctypes.data))
    return first


def coverage_windows(ctx, bam, all_reads, min_align_per, max_edit_dist_per, window_size, budget_bytes=0):
    """The device pass of CoverageWindows over every record of an open Bam (ckm_coverage_windows_run): ([n_ref, 9] int64 counters by the
    chain of coverageWindows.py, [n_ref + 1] first slots, [slots] int64 depth sums, timing dict).  Raises CoverageRecordError as
    coverage_counters() does, with reasons 5 (no CIGAR) and 6 (mapped read with pos < 0) besides."""
    p = _coverage_windows_params(all_reads, min_align_per, max_edit_dist_per, window_size, budget_bytes)
    _chk(load().ckm_coverage_windows_check(C.byref(p)))
    first = coverage_windows_layout(bam, window_size)
    out = np.zeros((max(1, len(bam.references)), len(COVERAGE_SLOTS)), dtype=np.int64)
    sums = np.zeros(max(1, int(first[-1])), dtype=np.int64)
    t = CoverageWindowsTiming()
    rc = load().ckm_coverage_windows_run(ctx.h, bam.h, C.byref(p), out.ctypes.data, sums.ctypes.data, C.byref(t))
    if rc != 0 and t.error_reason:
        raise CoverageRecordError(rc, load().ckm_last_error().decode(errors="replace"), int(t.error_reason), int(t.error_record), t.error_read.decode(errors="replace"))
    _chk(rc)
    timing = {f: getattr(t, f) for f in ("records", "batches", "blocks", "inflated_bytes", "slots", "ms_read", "ms_inflate", "ms_offsets", "ms_upload", "ms_kernel", "ms_scan",
                                         "ms_download", "ms_total")}
    return out[:len(bam.references)], first, sums[:int(first[-1])], timing


def seq_windows_layout(seqs, window_size):
    """first [nseq + 1] int64: the first window of every sequence of a NucSeqs batch and their number (ckm_seq_windows_layout):
    (L - 1) // window_size windows for a sequence of L > 0 code points.  O(sequences): the library counted the code points when it
    read the batch.  No device needed."""
    first = np.zeros(seqs.nseq + 1, dtype=np.int64)
    _chk(load().ckm_seq_windows_layout(seqs.h, int(window_size), first.ctypes.data))
    return first


def seq_lengths(seqs):
    """len(seq) of every sequence of a NucSeqs batch in code points, without decoding it: a sequence of L > 0 has L - 1 windows of one."""
    try:
        return [int(d) + (1 if n else 0) for d, n in zip(np.diff(seq_windows_layout(seqs, 1)).tolist(), seqs.seq_bytes.tolist())]
    except CkmError:                                       # more than 2^31 - 1 code points in the batch
        return [len(seqs.seq(i).decode('utf-8')) for i in range(seqs.nseq)]


def seq_windows(ctx, seqs, window_size, bin_sig=None, want_tetra=False, piece_bytes=0, budget_bytes=0):
    """The device pass over the windows of a NucSeqs batch (ckm_seq_windows_run).  bin_sig: [nfiles, 136] float64 or None.  Returns a
    dict: first [nseq + 1], base [nwin, 4] uint32 (A, C, G, T+U), seq [nseq, 4] uint64, td [nwin] float64 or None, tetra [nwin, 136]
    uint32 or None, skipped [nseq] bool (non-ASCII sequences, left to the caller), and the timings."""
    first = seq_windows_layout(seqs, window_size)
    nwin, nseq = int(first[-1]), seqs.nseq
    base = np.zeros((max(1, nwin), 4), dtype=np.uint32)
    per_seq = np.zeros((max(1, nseq), 4), dtype=np.uint64)
    skipped = np.zeros(max(1, nseq), dtype=np.uint8)
    td = tetra = sig = None
    if bin_sig is not None:
        sig = np.ascontiguousarray(bin_sig, dtype=np.float64)
        if sig.shape != (seqs.nfiles, 136):
            raise ValueError("bin_sig must be [nfiles, 136]")
        td = np.zeros(max(1, nwin), dtype=np.float64)
    if want_tetra:
        tetra = np.zeros((max(1, nwin), 136), dtype=np.uint32)
    t = SeqWindowsTiming()
    _chk(load().ckm_seq_windows_run(ctx.h, seqs.h, int(window_size), 1 if (sig is not None or want_tetra) else 0, sig.ctypes.data if sig is not None else None,
                                    int(piece_bytes), int(budget_bytes), base.ctypes.data, per_seq.ctypes.data, td.ctypes.data if td is not None else None,
                                    tetra.ctypes.data if tetra is not None else None, skipped.ctypes.data, C.byref(t)))
    out = dict(first=first, base=base[:nwin], seq=per_seq[:nseq], td=None if td is None else td[:nwin], tetra=None if tetra is None else tetra[:nwin],
               skipped=skipped[:nseq].astype(bool))
    out.update((f, getattr(t, f)) for f, _ in SeqWindowsTiming._fields_)
    return out


def seq_windows_coding(seqs, gff_paths, window_size):
    """(coding bases per window [nwin] int64, missing [nfiles] bool) from bins/<binId>/genes.gff of every file (ckm_seq_windows_coding):
    np.sum(codingBaseMask[k w:(k + 1) w]); -1 for the windows of a file without a GFF.  No device needed."""
    n = seqs.nfiles
    first = seq_windows_layout(seqs, window_size)
    g = (C.c_char_p * max(1, n))(*[os.fsencode(p) for p in gff_paths])
    coding = np.zeros(max(1, int(first[-1])), dtype=np.int64)
    missing = np.zeros(max(1, n), dtype=np.uint8)
    _chk(load().ckm_seq_windows_coding(g, seqs.h, int(window_size), coding.ctypes.data, missing.ctypes.data))
    return coding[:int(first[-1])], missing[:n].astype(bool)


REFDIST_STATS = {"gc": 0, "cd": 1, "td": 2}


def _refdist_windows(starts, sizes):
    a, w = np.ascontiguousarray(starts, dtype=np.int64), np.ascontiguousarray(sizes, dtype=np.int64)
    if a.ndim != 1 or a.shape != w.shape:
        raise ValueError("starts and sizes must be two lists of one length")
    return a, w


def refdist_check(stat, sep_len, block, scaffold_len, starts, sizes):
    """Raises CkmError for arguments ckm_refdist_run would refuse (ckm_refdist_check).  No device needed."""
    a, w = _refdist_windows(starts, sizes)
    _chk(load().ckm_refdist_check(int(stat), int(sep_len), int(block), int(scaffold_len), a.ctypes.data, w.ctypes.data, len(a)))


def refdist(ctx, seqs, stat, sep_len, starts, sizes, block=0, budget_bytes=0):
    """The device pass over windows [start, start + size) of the scaffold of a NucSeqs batch (ckm_refdist_run).  stat: 'gc', 'cd' or
    'td'.  Returns a dict: counts [nwin, 2] uint32 (gc, at) or None, td [nwin] float64 or None, totals [138] uint64 (gc, at, the 136
    canonical 4-mer counts of the scaffold), and the timings."""
    a, w = _refdist_windows(starts, sizes)
    n, code = len(a), REFDIST_STATS[stat]
    counts = np.zeros((max(1, n), 2), dtype=np.uint32) if code != 2 else None
    td = np.zeros(max(1, n), dtype=np.float64) if code == 2 else None
    totals = np.zeros(138, dtype=np.uint64)
    t = RefDistTiming()
    _chk(load().ckm_refdist_run(ctx.h, seqs.h, code, int(sep_len), int(block), a.ctypes.data, w.ctypes.data, n, int(budget_bytes),
                                counts.ctypes.data if counts is not None else None, td.ctypes.data if td is not None else None, totals.ctypes.data, C.byref(t)))
    out = dict(counts=None if counts is None else counts[:n], td=None if td is None else td[:n], totals=totals)
    out.update((f, getattr(t, f)) for f, _ in RefDistTiming._fields_)
    return out


def refdist_coding(gff_path, seq_id, starts, sizes):
    """(coding bases per window [nwin] int64, coding bases of the sequence) of sequence seq_id of a GFF (ckm_refdist_coding):
    ProdigalGeneFeatureParser.codingBases(seqId, start, start + size) and codingBases(seqId).  No device needed."""
    a, w = _refdist_windows(starts, sizes)
    coding = np.zeros(max(1, len(a)), dtype=np.int64)
    total = C.c_int64()
    _chk(load().ckm_refdist_coding(os.fsencode(gff_path), seq_id.encode("utf-8"), a.ctypes.data, w.ctypes.data, len(a), coding.ctypes.data, C.byref(total)))
    return coding[:len(a)], int(total.value)


class FastaIds(object):
    """The ids and lengths of FASTA files by the rules of NucSeqs, without their text (ckm_fasta_ids_read); stays in the library until
    close().  seq_bytes, seq_cp: bytes and code points of every sequence; file_first [nfiles + 1]."""

    def __init__(self, paths):
        arr = (C.c_char_p * max(1, len(paths)))(*[os.fsencode(p) for p in paths])
        self.h = C.c_void_p()
        _chk(load().ckm_fasta_ids_read(arr, len(paths), C.byref(self.h)))
        v = FastaIdsView()
        _chk(load().ckm_fasta_ids_view_get(self.h, C.byref(v)))
        self.nseq, self.nfiles = int(v.nseq), int(v.nfiles)
        arr = np.ctypeslib.as_array
        self.seq_bytes = arr(v.seq_bytes, shape=(self.nseq,)).copy() if self.nseq else np.zeros(0, dtype=np.uint64)
        self.seq_cp = arr(v.seq_cp, shape=(self.nseq,)).copy() if self.nseq else np.zeros(0, dtype=np.uint64)
        self.file_first = arr(v.file_first, shape=(self.nfiles + 1,)).copy()
        self._view = v

    def ids(self):
        return [self._view.seq_ids[i].decode("utf-8") for i in range(self.nseq)]

    def close(self):
        if self.h:
            load().ckm_fasta_ids_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def unbinned_select(bins, seqs, min_len):
    """(keep [nseq] uint8, totals dict) of an assembly read as NucSeqs against the ids of `bins` (a FastaIds, or None): keep = the id is
    in no bin and the sequence has at least min_len code points (ckm_unbinned_select).  seqs = None: the totals of the bins alone and
    no keep.  No device needed."""
    nseq = seqs.nseq if seqs is not None else 0
    keep = np.zeros(max(1, nseq), dtype=np.uint8)
    t = UnbinnedTotals()
    _chk(load().ckm_unbinned_select(bins.h if bins is not None else None, seqs.h if seqs is not None else None, int(min_len), keep.ctypes.data, C.byref(t)))
    return (keep[:nseq] if seqs is not None else None), dict((f, int(getattr(t, f))) for f, _ in UnbinnedTotals._fields_)


def unbinned_count(ctx, seqs, keep, tile_bytes=0, budget_bytes=0):
    """The device count over the kept sequences of a NucSeqs batch (ckm_unbinned_count).  Returns a dict: counts [nseq, 5] uint64 (A, C,
    G, T+U, code points; zeros where keep is 0) and the timings."""
    keep = np.ascontiguousarray(keep, dtype=np.uint8)
    assert keep.shape == (seqs.nseq,)
    counts = np.zeros((max(1, seqs.nseq), 5), dtype=np.uint64)
    t = UnbinnedTiming()
    _chk(load().ckm_unbinned_count(ctx.h, seqs.h, keep.ctypes.data if seqs.nseq else counts.ctypes.data, int(tile_bytes), int(budget_bytes), counts.ctypes.data, C.byref(t)))
    out = dict(counts=counts[:seqs.nseq])
    out.update((f, getattr(t, f)) for f, _ in UnbinnedTiming._fields_)
    return out


def unbinned_write(seqs, keep, counts, seq_path, stats_path):
    """The two files of Unbinned.run written by the library from the batch's own buffers (ckm_unbinned_write).  Returns the index of the
    kept sequence without A, C, G, T or U at which the writing stopped (its FASTA record written, its row not), or -1."""
    keep = np.ascontiguousarray(keep, dtype=np.uint8)
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    assert keep.shape == (seqs.nseq,) and counts.shape == (seqs.nseq, 5)
    zero = C.c_int64(-1)
    _chk(load().ckm_unbinned_write(seqs.h, keep.ctypes.data if seqs.nseq else None, counts.ctypes.data if seqs.nseq else None, os.fsencode(seq_path),
                                   os.fsencode(stats_path), C.byref(zero)))
    return int(zero.value)


def _aai_args(groups):
    """(group_row_off, row_off, text) of groups given as sequences of rows (bytes, or str of ASCII): the rows back to back."""
    rows = [r if isinstance(r, bytes) else r.encode("ascii") for g in groups for r in g]
    group_row_off = np.zeros(len(groups) + 1, dtype=np.uint64)
    np.cumsum([len(g) for g in groups], out=group_row_off[1:])
    row_off = np.zeros(len(rows) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in rows], out=row_off[1:])
    return group_row_off, row_off, b"".join(rows)


def aai_check(groups):
    """ckm_aai_check: the argument tests of aai_pairs(), without a device.  Raises CkmError as aai_pairs would."""
    group_row_off, row_off, text = _aai_args(groups)
    _chk(load().ckm_aai_check(len(groups), group_row_off.ctypes.data, row_off.ctypes.data, text))


def aai_pairs(ctx, groups, budget_bytes=0):
    """Amino-acid identity between all pairs of rows of every group (ckm_aai_run): groups is a sequence of groups, a group a sequence
    of rows of equal length (bytes, or str of ASCII).  Returns a dict: pair_off [ngroups + 1] uint64, and per pair i < j (i major, groups
    in order) mismatches and compared (int32) and aai (float64); npairs, nbatches, bytes and the timings in ms."""
    group_row_off, row_off, text = _aai_args(groups)
    h = C.c_void_p()
    _chk(load().ckm_aai_run(ctx.h, len(groups), group_row_off.ctypes.data, row_off.ctypes.data, text, int(budget_bytes), C.byref(h)))
    try:
        c = AaiColumns()
        _chk(load().ckm_aai_columns_get(h, C.byref(c)))
        k = int(c.npairs)
        arr = np.ctypeslib.as_array
        out = dict(npairs=k, nbatches=int(c.nbatches), bytes=int(c.bytes), pair_off=arr(c.pair_off, shape=(len(groups) + 1,)).copy())
        for f, dt in (("mismatches", np.int32), ("compared", np.int32), ("aai", np.float64)):
            out[f] = arr(getattr(c, f), shape=(k,)).copy() if k else np.zeros(0, dtype=dt)
        for f in ("ms_pack", "ms_upload", "ms_kernel", "ms_download", "ms_total"):
            out[f] = getattr(c, f)
    finally:
        load().ckm_aai_free(h)
    return out


def _mset_table_args(count_class, pos_off, pos):
    """(ngenomes, nfamilies, classes uint8 [G, C], pos_off uint64 [G * C + 1], pos int64) of a table given as arrays."""
    cls = np.ascontiguousarray(count_class, dtype=np.uint8)
    if cls.ndim != 2:
        raise ValueError("count_class must be [ngenomes, nfamilies]")
    off = np.ascontiguousarray(pos_off, dtype=np.uint64).reshape(-1)
    if off.shape[0] != cls.shape[0] * cls.shape[1] + 1:
        raise ValueError("pos_off must hold ngenomes * nfamilies + 1 entries")
    return cls.shape[0], cls.shape[1], cls, off, np.ascontiguousarray(pos, dtype=np.int64).reshape(-1)


def _mset_lists(lists):
    """(offsets uint64 [n + 1], members uint32) of a sequence of index lists."""
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    flat = np.concatenate([np.asarray(x, dtype=np.int64).reshape(-1) for x in lists]) if len(lists) else np.zeros(0, dtype=np.int64)
    if flat.size and (flat.min() < 0 or flat.max() > 0xFFFFFFFF):
        raise CkmError(-1, "an index that does not fit uint32")
    return off, np.ascontiguousarray(flat, dtype=np.uint32)


def _ptr(a):
    return a.ctypes.data if a.size else None


def mset_check(count_class, pos_off, pos, genome_lists=None, marker_lists=None, dist_threshold=5000):
    """ckm_mset_check: why a table, the queries of a call or a distance threshold would be refused, without a device.  Raises CkmError
    as MsetTable / mset_markers / mset_colocated would."""
    G, Cn, cls, off, p = _mset_table_args(count_class, pos_off, pos)
    goff, g = _mset_lists(genome_lists) if genome_lists is not None else (None, None)
    moff, m = _mset_lists(marker_lists) if marker_lists is not None else (None, None)
    _chk(load().ckm_mset_check(G, Cn, _ptr(cls), off.ctypes.data, _ptr(p), len(genome_lists) if genome_lists is not None else 0,
                               goff.ctypes.data if goff is not None else None, _ptr(g) if g is not None else None,
                               moff.ctypes.data if moff is not None else None, _ptr(m) if m is not None else None, float(dist_threshold)))


class MsetTable(object):
    """The resident table of MarkerSetBuilder (ckm_mset_table_create): count_class [ngenomes, nfamilies] of 0 / 1 / 2, and the copy
    positions of every (genome, family) cell as pos[pos_off[cell] : pos_off[cell + 1]], cells genome-major."""

    def __init__(self, ctx, count_class, pos_off, pos):
        self.ngenomes, self.nfamilies, cls, off, p = _mset_table_args(count_class, pos_off, pos)
        self.ctx = ctx
        self.h = C.c_void_p()
        ms = C.c_double(0.0)
        _chk(load().ckm_mset_table_create(ctx.h, self.ngenomes, self.nfamilies, _ptr(cls), off.ctypes.data, _ptr(p), C.byref(ms), C.byref(self.h)))
        self.ms_upload = ms.value

    def close(self):
        if self.h:
            load().ckm_mset_table_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:          # interpreter shutdown: the library may be gone already
            pass


_MSET_MS = ("ms_upload", "ms_markers", "ms_pack", "ms_count", "ms_scan", "ms_fill", "ms_download", "ms_total")


def mset_markers(ctx, table, genome_lists, ubiquity_thresholds, single_copy_thresholds, want_counts=False, budget_bytes=0):
    """The marker pass (ckm_mset_markers) over a batch of queries: genome_lists are lists of genome indices of the table, the thresholds
    the doubles the caller computed.  Returns a dict: flag [nqueries, nfamilies] uint8 (bit 0 marker, bit 1 missing, bit 2 duplicate),
    counts [nqueries, nfamilies, 3] uint32 (ubiquity, single, duplicate) or None, nbatches and the timings in ms."""
    goff, g = _mset_lists(genome_lists)
    tu = np.ascontiguousarray(ubiquity_thresholds, dtype=np.float64).reshape(-1)
    ts = np.ascontiguousarray(single_copy_thresholds, dtype=np.float64).reshape(-1)
    nq = len(genome_lists)
    if tu.shape[0] != nq or ts.shape[0] != nq:
        raise ValueError("one threshold pair per query")
    h = C.c_void_p()
    _chk(load().ckm_mset_markers(ctx.h, table.h, nq, goff.ctypes.data, _ptr(g), _ptr(tu), _ptr(ts), 1 if want_counts else 0, int(budget_bytes), C.byref(h)))
    try:
        c = MsetColumns()
        _chk(load().ckm_mset_columns_get(h, C.byref(c)))
        n = nq * table.nfamilies
        arr = np.ctypeslib.as_array
        out = dict(nbatches=int(c.nbatches), flag=(arr(c.flag, shape=(n,)).copy() if n else np.zeros(0, dtype=np.uint8)).reshape(nq, table.nfamilies), counts=None)
        if want_counts:
            out["counts"] = (arr(c.counts, shape=(n * 3,)).copy() if n else np.zeros(0, dtype=np.uint32)).reshape(nq, table.nfamilies, 3)
        for f in _MSET_MS:
            out[f] = getattr(c, f)
    finally:
        load().ckm_mset_result_free(h)
    return out


def mset_colocated(ctx, table, genome_lists, marker_lists, dist_threshold=5000, genome_threshold=0.95, budget_bytes=0):
    """The co-location pass (ckm_mset_colocated) over a batch of queries: per query a list of genome indices and a list of family indices
    (its markers).  Returns a dict: pair_off [nqueries + 1] uint64 and per reported pair, in ascending (i, j) per query, i and j
    (positions in the query's marker list) and count (genomes), uint32; npairs, nbatches, nrounds, tests and the timings in ms."""
    if len(genome_lists) != len(marker_lists):
        raise ValueError("one marker list per query")
    goff, g = _mset_lists(genome_lists)
    moff, m = _mset_lists(marker_lists)
    nq = len(genome_lists)
    h = C.c_void_p()
    _chk(load().ckm_mset_colocated(ctx.h, table.h, nq, goff.ctypes.data, _ptr(g), moff.ctypes.data, _ptr(m), float(dist_threshold), float(genome_threshold),
                                   int(budget_bytes), C.byref(h)))
    try:
        c = MsetColumns()
        _chk(load().ckm_mset_columns_get(h, C.byref(c)))
        k = int(c.npairs)
        arr = np.ctypeslib.as_array
        out = dict(npairs=k, nbatches=int(c.nbatches), nrounds=int(c.nrounds), tests=int(c.tests), pair_off=arr(c.pair_off, shape=(nq + 1,)).copy())
        for f in ("i", "j", "count"):
            out[f] = arr(getattr(c, f), shape=(k,)).copy() if k else np.zeros(0, dtype=np.uint32)
        for f in _MSET_MS:
            out[f] = getattr(c, f)
    finally:
        load().ckm_mset_result_free(h)
    return out


class SimTables(object):
    """The arrays of one simulation call as ckm_sim_check / ckm_sim_run take them (include/checkm_hip.h): key_off / key for the distinct
    markers, ms_off / cs_off / cs_marker for the marker sets, rs_off / starts / contig_len for the replicates.  Keys, starts and contig
    lengths are int64 here; the library checks them down to int32."""

    def __init__(self, key_off, key, ms_off, cs_off, cs_marker, rs_off, starts, contig_len):
        u64 = lambda x: np.ascontiguousarray(x, dtype=np.uint64).reshape(-1)
        i64 = lambda x: np.ascontiguousarray(x, dtype=np.int64).reshape(-1)
        self.key_off, self.key, self.ms_off, self.cs_off, self.rs_off = u64(key_off), i64(key), u64(ms_off), u64(cs_off), u64(rs_off)
        self.cs_marker = np.ascontiguousarray(cs_marker, dtype=np.uint32).reshape(-1)
        self.starts, self.contig_len = i64(starts), i64(contig_len)
        if not (self.key_off.size and self.ms_off.size and self.cs_off.size and self.rs_off.size):
            raise ValueError("an offset table holds at least its leading 0")
        if self.contig_len.shape[0] != self.rs_off.shape[0] - 1:
            raise ValueError("one contig length per replicate")
        self.nmarkers, self.nsets, self.nreplicates = self.key_off.shape[0] - 1, self.ms_off.shape[0] - 1, self.rs_off.shape[0] - 1

    def args(self):
        """The ckm_sim_args of these arrays (it borrows them: keep this object alive over the call)."""
        return SimArgs(self.nmarkers, self.key_off.ctypes.data, _ptr(self.key), self.key.shape[0],
                       self.nsets, self.ms_off.ctypes.data, self.cs_off.ctypes.data, self.cs_off.shape[0] - 1, _ptr(self.cs_marker), self.cs_marker.shape[0],
                       self.nreplicates, self.rs_off.ctypes.data, _ptr(self.starts), self.starts.shape[0], _ptr(self.contig_len))


def sim_check(tables):
    """ckm_sim_check: why the keys, the marker sets or the replicates of a call would be refused, without a device.  Raises CkmError as
    sim_run would."""
    a = tables.args()
    _chk(load().ckm_sim_check(C.byref(a)))


def sim_run(ctx, tables, budget_bytes=0):
    """The simulation pass (ckm_sim_run) over all replicates of a call.  Returns a dict: out [nreplicates, nsets, 4] float64 (individual
    completeness and contamination, set completeness and contamination, in percent), nrounds and the timings in ms."""
    out = np.zeros((tables.nreplicates, tables.nsets, 4), dtype=np.float64)
    info, a = SimInfo(), tables.args()
    _chk(load().ckm_sim_run(ctx.h, C.byref(a), int(budget_bytes), _ptr(out), C.byref(info)))
    return dict(out=out, nrounds=int(info.nrounds), **{f: getattr(info, f) for f in ("ms_pack", "ms_upload", "ms_kernel", "ms_download", "ms_total")})


SIMSCAF_NONE = 0xffffffff


class SimScafTables(object):
    """The arrays of one scaffold-simulation call as ckm_simscaf_check / ckm_simscaf_run take them (include/checkm_hip.h): nscaf per
    genome, sc_off / sc for the (genome, marker) cells, ms_off / cs_off / cs_marker for the marker sets, test / cont / bit_off / bits for
    the replicates (cont SIMSCAF_NONE: no contaminant)."""

    def __init__(self, nscaf, nmarkers, sc_off, sc, ms_off, cs_off, cs_marker, test, cont, bit_off, bits):
        u64 = lambda x: np.ascontiguousarray(x, dtype=np.uint64).reshape(-1)
        u32 = lambda x: np.ascontiguousarray(x, dtype=np.uint32).reshape(-1)
        self.nscaf, self.sc, self.cs_marker, self.test, self.cont, self.bits = u32(nscaf), u32(sc), u32(cs_marker), u32(test), u32(cont), u32(bits)
        self.sc_off, self.ms_off, self.cs_off, self.bit_off = u64(sc_off), u64(ms_off), u64(cs_off), u64(bit_off)
        self.ngenomes, self.nmarkers = self.nscaf.shape[0], int(nmarkers)
        if not (self.ms_off.size and self.cs_off.size and self.bit_off.size):
            raise ValueError("an offset table holds at least its leading 0")
        if self.sc_off.shape[0] != self.ngenomes * self.nmarkers + 1:
            raise ValueError("one offset per (genome, marker) cell and the end")
        if not (self.test.shape[0] == self.cont.shape[0] == self.bit_off.shape[0] - 1):
            raise ValueError("one test genome, one contaminant and one offset per replicate")
        self.nsets, self.nreplicates = self.ms_off.shape[0] - 1, self.test.shape[0]

    def args(self):
        """The ckm_simscaf_args of these arrays (it borrows them: keep this object alive over the call)."""
        return SimScafArgs(self.ngenomes, _ptr(self.nscaf), self.nmarkers, self.sc_off.ctypes.data, _ptr(self.sc), self.sc.shape[0],
                           self.nsets, self.ms_off.ctypes.data, self.cs_off.ctypes.data, self.cs_off.shape[0] - 1, _ptr(self.cs_marker), self.cs_marker.shape[0],
                           self.nreplicates, _ptr(self.test), _ptr(self.cont), self.bit_off.ctypes.data, _ptr(self.bits), self.bits.shape[0])


def simscaf_check(tables):
    """ckm_simscaf_check: why the tables, the marker sets or the replicates of a call would be refused, without a device.  Raises
    CkmError as simscaf_run would."""
    a = tables.args()
    _chk(load().ckm_simscaf_check(C.byref(a)))


def simscaf_run(ctx, tables, budget_bytes=0):
    """The scaffold-simulation pass (ckm_simscaf_run) over all replicates of a call.  Returns a dict: out [nreplicates, nsets, 4] float64
    (individual completeness and contamination, set completeness and contamination, in percent), nrounds and the timings in ms."""
    out = np.zeros((tables.nreplicates, tables.nsets, 4), dtype=np.float64)
    info, a = SimInfo(), tables.args()
    _chk(load().ckm_simscaf_run(ctx.h, C.byref(a), int(budget_bytes), _ptr(out), C.byref(info)))
    return dict(out=out, nrounds=int(info.nrounds), **{f: getattr(info, f) for f in ("ms_pack", "ms_upload", "ms_kernel", "ms_download", "ms_total")})


class SelectTables(object):
    """The arrays of one selection call as ckm_select_check / ckm_select_run take them (include/checkm_hip.h): genome_len per test genome,
    key_off / key for the (genome, marker) cells, ms_off / cs_off / cs_marker for the marker sets, the replicates per genome, the contig
    length, the two ranges and the seed.  Keys and lengths are int64 here; the library checks them down to int32."""

    def __init__(self, genome_len, nmarkers, key_off, key, ms_off, cs_off, cs_marker, nreplicates, contig_len, comp_range, cont_range, seed):
        u64 = lambda x: np.ascontiguousarray(x, dtype=np.uint64).reshape(-1)
        i64 = lambda x: np.ascontiguousarray(x, dtype=np.int64).reshape(-1)
        self.genome_len, self.key_off, self.key, self.ms_off, self.cs_off = i64(genome_len), u64(key_off), i64(key), u64(ms_off), u64(cs_off)
        self.cs_marker = np.ascontiguousarray(cs_marker, dtype=np.uint32).reshape(-1)
        self.ngenomes, self.nmarkers, self.nreplicates, self.contig_len = self.genome_len.shape[0], int(nmarkers), int(nreplicates), int(contig_len)
        if not (self.ms_off.size and self.cs_off.size):
            raise ValueError("an offset table holds at least its leading 0")
        if self.key_off.shape[0] != self.ngenomes * self.nmarkers + 1:
            raise ValueError("one offset per (genome, marker) cell and the end")
        self.nsets = self.ms_off.shape[0] - 1
        (self.comp_lo, self.comp_hi), (self.cont_lo, self.cont_hi) = (float(x) for x in comp_range), (float(x) for x in cont_range)
        self.seed = int(seed) & 0xffffffffffffffff

    def args(self):
        """The ckm_select_args of these arrays (it borrows them: keep this object alive over the call)."""
        return SelectArgs(self.ngenomes, _ptr(self.genome_len), self.nmarkers, self.key_off.ctypes.data, _ptr(self.key), self.key.shape[0],
                          self.nsets, self.ms_off.ctypes.data, self.cs_off.ctypes.data, self.cs_off.shape[0] - 1, _ptr(self.cs_marker), self.cs_marker.shape[0],
                          self.nreplicates, self.contig_len, self.comp_lo, self.comp_hi, self.cont_lo, self.cont_hi, self.seed)

    def ncontigs(self):
        """C_g of every genome (of a call that passed select_check)."""
        return [int(n) // self.contig_len for n in self.genome_len]


def select_check(tables):
    """ckm_select_check: why the genomes, the keys, the marker sets or the ranges of a call would be refused, without a device.  Raises
    CkmError as select_run would."""
    a = tables.args()
    _chk(load().ckm_select_check(C.byref(a)))


def select_arrays(tables, with_rows):
    """The result arrays of a call: truth [G, R, 2], out [G, R, S, 4] and, on request, the flat uint16 multiplicity rows."""
    truth = np.zeros((tables.ngenomes, tables.nreplicates, 2), dtype=np.float64)
    out = np.zeros((tables.ngenomes, tables.nreplicates, tables.nsets, 4), dtype=np.float64)
    rows = np.zeros(sum(tables.ncontigs()) * tables.nreplicates, dtype=np.uint16) if with_rows else None
    return truth, out, rows


def select_rows(tables, rows):
    """The flat multiplicity rows as one array [R, C_g] per genome."""
    split, at = [], 0
    for c in tables.ncontigs():
        split.append(rows[at:at + tables.nreplicates * c].reshape(tables.nreplicates, c))
        at += tables.nreplicates * c
    return split


def select_run(ctx, tables, budget_bytes=0, with_rows=False):
    """The selection pass (ckm_select_run) over all draws of a call.  Returns a dict: truth [ngenomes, nreplicates, 2] float64 (true
    completeness and contamination of every draw, in percent), out [ngenomes, nreplicates, nsets, 4] float64 as sim_run's, rows (with_rows:
    per genome the uint16 multiplicities [nreplicates, C_g], else None), nrounds and the timings in ms."""
    info, a = SimInfo(), tables.args()
    truth, out, rows = select_arrays(tables, with_rows)
    o = SelectOut(_ptr(truth), _ptr(out), _ptr(rows) if with_rows else None)
    _chk(load().ckm_select_run(ctx.h, C.byref(a), int(budget_bytes), C.byref(o), C.byref(info)))
    return dict(truth=truth, out=out, rows=select_rows(tables, rows) if with_rows else None, nrounds=int(info.nrounds),
                **{f: getattr(info, f) for f in ("ms_pack", "ms_upload", "ms_kernel", "ms_download", "ms_total")})


class PlaceTables(object):
    """The arrays of one placement call as ckm_place_check / ckm_place_run take them (include/checkm_hip.h): the tree as children lists
    (child_off / child) with the length of the edge above every node, the reference alignment (one row of bytes per leaf, ascending node
    order) and the queries with their offsets, the rate weights, the eigenvectors U / Uinv, the frequencies pi and the host-made tables
    of exponentials exp_len [N, R, 20], exp_half [N, R, 20], exp_dist [N, F, 2, R, 20] and exp_pend [1 + G, R, 20]."""

    def __init__(self, child_off, child, length, nsites, row_off, rows, q_off, queries, weights, U, Uinv, pi, exp_len, exp_half, exp_dist, exp_pend, max_pitches):
        u64 = lambda x: np.ascontiguousarray(x, dtype=np.uint64).reshape(-1)
        f64 = lambda x: np.ascontiguousarray(x, dtype=np.float64)
        u8 = lambda x: np.ascontiguousarray(np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=np.uint8).reshape(-1)
        self.child_off, self.row_off, self.q_off = u64(child_off), u64(row_off), u64(q_off)
        self.child = np.ascontiguousarray(child, dtype=np.uint32).reshape(-1)
        self.length, self.weights, self.U, self.Uinv, self.pi = f64(length).reshape(-1), f64(weights).reshape(-1), f64(U), f64(Uinv), f64(pi).reshape(-1)
        self.rows, self.queries = u8(rows), u8(queries)
        self.exp_len, self.exp_half, self.exp_dist, self.exp_pend = f64(exp_len), f64(exp_half), f64(exp_dist), f64(exp_pend)
        if not (self.child_off.size and self.row_off.size and self.q_off.size):
            raise ValueError("an offset table holds at least its leading 0")
        self.nnodes, self.nrows, self.nqueries = self.child_off.shape[0] - 1, self.row_off.shape[0] - 1, self.q_off.shape[0] - 1
        self.nsites, self.nrates, self.max_pitches = int(nsites), self.weights.shape[0], int(max_pitches)
        if self.length.shape[0] != self.nnodes or self.U.shape != (20, 20) or self.Uinv.shape != (20, 20) or self.pi.shape[0] != 20:
            raise ValueError("one length per node, 20 x 20 eigenvectors and 20 frequencies")
        if self.exp_len.shape != (self.nnodes, self.nrates, 20) or self.exp_half.shape != self.exp_len.shape:
            raise ValueError("exp_len and exp_half are [nodes, rates, 20]")
        if self.exp_dist.ndim != 5 or self.exp_dist.shape[:1] + self.exp_dist.shape[2:] != (self.nnodes, 2, self.nrates, 20):
            raise ValueError("exp_dist is [nodes, fractions, 2, rates, 20]")
        if self.exp_pend.ndim != 3 or self.exp_pend.shape[0] < 1 or self.exp_pend.shape[1:] != (self.nrates, 20):
            raise ValueError("exp_pend is [1 + pendant lengths, rates, 20]")
        self.nfrac, self.npend = self.exp_dist.shape[1], self.exp_pend.shape[0] - 1

    def args(self):
        """The ckm_place_args of these arrays (it borrows them: keep this object alive over the call)."""
        return PlaceArgs(self.nnodes, self.child_off.ctypes.data, _ptr(self.child), self.child.shape[0], _ptr(self.length),
                         self.nsites, self.nrows, self.row_off.ctypes.data, _ptr(self.rows), self.rows.shape[0],
                         self.nqueries, self.q_off.ctypes.data, _ptr(self.queries), self.queries.shape[0],
                         self.nrates, _ptr(self.weights), _ptr(self.U), _ptr(self.Uinv), _ptr(self.pi), _ptr(self.exp_len), _ptr(self.exp_half),
                         self.nfrac, _ptr(self.exp_dist), self.npend, _ptr(self.exp_pend), self.max_pitches)

    def outputs(self):
        """Fresh output arrays [nqueries, max_pitches] and the ckm_place_out over them."""
        shape = (self.nqueries, self.max_pitches)
        o = dict(top_edge=np.full(shape, -1, dtype=np.int32), scan_m=np.zeros(shape), scan_e=np.zeros(shape, dtype=np.int64), ref_m=np.zeros(shape),
                 ref_e=np.zeros(shape, dtype=np.int64), ref_f=np.full(shape, -1, dtype=np.int32), ref_g=np.full(shape, -1, dtype=np.int32))
        return o, PlaceOut(*[_ptr(o[f]) for f in ("top_edge", "scan_m", "scan_e", "ref_m", "ref_e", "ref_f", "ref_g")])


def place_check(tables):
    """ckm_place_check: why the tree, the alignment, the queries or the tables of a call would be refused, without a device.  Raises
    CkmError as place_run would."""
    a = tables.args()
    _chk(load().ckm_place_check(C.byref(a)))


def place_run(ctx, tables, budget_bytes=0):
    """The placement pass (ckm_place_run).  Returns a dict: per (query, kept slot) top_edge (int32, -1 beyond the edges), the scan's
    likelihood scan_m * 2^scan_e, the refined ref_m * 2^ref_e with the grid indices ref_f / ref_g; nchunks, chunk_sites, the numbers of
    sweep levels and the timings in ms."""
    o, po = tables.outputs()
    info, a = PlaceInfo(), tables.args()
    _chk(load().ckm_place_run(ctx.h, C.byref(a), int(budget_bytes), C.byref(po), C.byref(info)))
    o.update({f: int(getattr(info, f)) for f in ("nchunks", "chunk_sites", "nlevels_up", "nlevels_down")})
    o.update({f: getattr(info, f) for f in _PLACE_MS})
    return o


class NhmmTables(object):
    """The arrays of one model scan as ckm_nhmm_check / ckm_nhmm_run take them (include/checkm_hip.h): per model the int32 milli-bit
    tables emis [4, M] (A C G T/U) and trans [7, M] (MM IM DM MI II MD DD, node k at index k - 1, the transitions into k holding node
    k - 1's numbers) and the reporting threshold min_score; the tile geometry stride / overlap; strands (1 forward, 2 reverse, 3 both)."""

    def __init__(self, models, min_score, stride, overlap, strands=3):
        for e, t in models:
            if e.ndim != 2 or t.ndim != 2 or e.shape[0] != 4 or t.shape[0] != 7 or t.shape[1] != e.shape[1]:
                raise ValueError("a model is (emis [4, M], trans [7, M])")
        self.M = np.ascontiguousarray([e.shape[1] for e, _ in models], dtype=np.uint32)
        self.tab_off = np.concatenate([[0], np.cumsum(self.M, dtype=np.uint64)]).astype(np.uint64)
        self.emis = np.ascontiguousarray(np.concatenate([np.asarray(e, dtype=np.int32).reshape(-1) for e, _ in models] or [np.zeros(0, dtype=np.int32)]), dtype=np.int32)
        self.trans = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int32).reshape(-1) for _, t in models] or [np.zeros(0, dtype=np.int32)]), dtype=np.int32)
        self.min_score = np.ascontiguousarray(min_score, dtype=np.int32).reshape(-1)
        if self.min_score.shape[0] != len(models):
            raise ValueError("one min_score per model")
        self.nmodels, self.stride, self.overlap, self.strands = len(models), int(stride), int(overlap), int(strands)

    def args(self):
        """The ckm_nhmm_args of these arrays (it borrows them: keep this object alive over the call)."""
        return NhmmArgs(self.nmodels, _ptr(self.M), self.tab_off.ctypes.data, _ptr(self.emis), _ptr(self.trans), int(self.tab_off[-1]), _ptr(self.min_score),
                        self.stride, self.overlap, self.strands)


def nhmm_columns(c, info):
    """The dict nhmm_run returns, copied out of a filled NhmmColumns and an info object with the NhmmInfo field names."""
    def col(p, n, dt):
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32 if dt == np.int32 else C.c_uint32)), shape=(n,)).copy() if n else np.zeros(0, dtype=dt)
    o = {f: col(getattr(c, f), int(c.nrows), np.int32 if f.endswith("score") else np.uint32) for f in _NHMM_ROWS}
    o.update({f: col(getattr(c, f), int(c.nhits), np.int32 if f.endswith("score") else np.uint32) for f in _NHMM_HITS})
    o.update({f: int(getattr(info, f)) for f in ("tiles", "launches", "cells", "batches")})
    o.update({f: float(getattr(info, f)) for f in _NHMM_MS})
    return o


def nhmm_check(tables):
    """ckm_nhmm_check: why the models, the thresholds or the geometry of a call would be refused, without a device.  Raises CkmError as
    nhmm_run would."""
    a = tables.args()
    _chk(load().ckm_nhmm_check(C.byref(a)))


def nhmm_run(ctx, tables, seqs, budget_bytes=0):
    """The model scan over a NucSeqs batch (ckm_nhmm_run).  Returns a dict: the reported rows (row_model, row_seq, row_strand, row_pos,
    row_start in strand coordinates, row_score), the hits (hit_model, hit_seq, hit_strand, hit_from <= hit_to on the forward strand,
    hit_score), tiles, launches, cells, batches and the timings in ms."""
    h, info, a = C.c_void_p(), NhmmInfo(), tables.args()
    _chk(load().ckm_nhmm_run(ctx.h, C.byref(a), seqs.h, int(budget_bytes), C.byref(h), C.byref(info)))
    try:
        c = NhmmColumns()
        _chk(load().ckm_nhmm_columns_get(h, C.byref(c)))
        return nhmm_columns(c, info)
    finally:
        load().ckm_nhmm_free(h)


GTREE_MODELS = {"kimura": 0, "poisson": 1, "p": 2}
GTREE_MAX_ROWS, GTREE_MAX_COLS = 1 << 14, 1 << 20


class GtreeTables(object):
    """The arrays of one genome-tree call as ckm_gtree_check / ckm_gtree_run take them (include/checkm_hip.h).  Either an alignment --
    text: nrows rows of ncols bytes in one uint8 array, cols: the drawn columns of the replicates [nreps, ncols] (or None), base: whether
    the alignment itself is the first tree, model: 0 / 1 / 2 or its name, max_dist -- or matrices [ntrees, nrows, nrows] float64."""

    def __init__(self, text=None, nrows=0, ncols=0, cols=None, base=True, model="kimura", max_dist=3.0, matrices=None):
        self.matrices = self.text = self.cols = None
        self.nreps, self.base, self.max_dist = 0, 1 if base else 0, float(max_dist)
        self.model = GTREE_MODELS[model] if model in GTREE_MODELS else int(model)
        if matrices is not None:
            self.matrices = np.ascontiguousarray(matrices, dtype=np.float64)
            if self.matrices.ndim != 3 or self.matrices.shape[1] != self.matrices.shape[2]:
                raise ValueError("matrices are [trees, rows, rows]")
            self.nrows, self.ncols, self.ntrees = self.matrices.shape[1], 0, self.matrices.shape[0]
            return
        self.text = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8).reshape(-1)
        self.nrows, self.ncols = int(nrows), int(ncols)
        if cols is not None:
            self.cols = np.ascontiguousarray(cols, dtype=np.uint32).reshape(-1, self.ncols if self.ncols else 1)
            self.nreps = self.cols.shape[0]
        self.ntrees = self.base + self.nreps

    def args(self):
        """The ckm_gtree_args of these arrays (it borrows them: keep this object alive over the call)."""
        if self.matrices is not None:
            return GtreeArgs(self.nrows, 0, None, 0, 0, None, 0, 0, self.max_dist, self.matrices.ctypes.data, self.ntrees)
        return GtreeArgs(self.nrows, self.ncols, _ptr(self.text), self.text.shape[0], self.nreps, _ptr(self.cols) if self.nreps else None, self.base, self.model, self.max_dist,
                         None, 0)


def gtree_check(tables):
    """ckm_gtree_check: why the alignment, the drawn columns, the model or the matrices of a call would be refused, without a device.
    Raises CkmError as gtree_run would."""
    a = tables.args()
    _chk(load().ckm_gtree_check(C.byref(a)))


def _gtree_call(entry, tables, budget_bytes, counts, dist, merges):
    a = tables.args()
    _chk(load().ckm_gtree_check(C.byref(a)))                  # (the output shapes below need a call that is in range)
    N, T = tables.nrows, tables.ntrees
    with_text = tables.matrices is None
    o = dict(compared=np.zeros((N, N), dtype=np.uint32) if counts and with_text else None, differ=np.zeros((N, N), dtype=np.uint32) if counts and with_text else None,
             dist=np.zeros((N, N)) if dist and with_text else None, merge_ij=np.zeros((T, N - 1, 2), dtype=np.uint32) if merges else None,
             merge_len=np.zeros((T, N - 1, 2)) if merges else None)
    info = GtreeInfo()
    go = GtreeOut(*[o[f].ctypes.data if o[f] is not None and o[f].size else None for f in ("compared", "differ", "dist", "merge_ij", "merge_len")])
    _chk(entry(C.byref(a), int(budget_bytes), C.byref(go), C.byref(info)))
    o.update({f: int(getattr(info, f)) for f in ("nrounds", "ntrees", "launches")})
    o.update({f: getattr(info, f) for f in _GTREE_MS})
    return o


def gtree_run(ctx, tables, budget_bytes=0, counts=False, dist=False, merges=True):
    """The genome-tree pass (ckm_gtree_run).  Returns a dict: compared, differ [nrows, nrows] uint32 (counts) and dist [nrows, nrows]
    float64 (dist) of the alignment itself, merge_ij [trees, nrows - 1, 2] uint32 and merge_len [trees, nrows - 1, 2] float64 (merges);
    what was not asked for is None; nrounds, ntrees, launches and the timings in ms."""
    L = load()
    return _gtree_call(lambda a, b, o, i: L.ckm_gtree_run(ctx.h, a, b, o, i), tables, budget_bytes, counts, dist, merges)


def gtree_host(tables, budget_bytes=0, counts=False, dist=False, merges=True):
    """The same call through the host executor (ckm_gtree_host): the same bits, no device.  For checks and comparisons; nothing in the
    package calls it in place of the device."""
    return _gtree_call(load().ckm_gtree_host, tables, budget_bytes, counts, dist, merges)


GENETREE_MAX_LEAVES, GENETREE_MAX_NODES, GENETREE_MAX_CLASSES = 1 << 14, 1 << 15, 65535
GENETREE_NONE = 0xffffffff
_GENETREE_FIELDS = (("node_off", np.uint32), ("leaf_off", np.uint32), ("class_off", np.uint32), ("group_off", np.uint32), ("gpair_off", np.uint32), ("first", np.uint32),
                    ("last", np.uint32), ("parent", np.uint32), ("length", np.float64), ("internal", np.uint8), ("leaf_genome", np.uint32), ("leaf_species", np.uint32),
                    ("leaf_class", np.uint32), ("class_total", np.uint32), ("pair_a", np.uint32), ("pair_b", np.uint32))


class GenetreeTables(object):
    """The packed forest of one gene-tree call as ckm_genetree_check / ckm_genetree_run take it (include/checkm_hip.h): node_off, leaf_off,
    group_off [ntrees + 1], class_off [3 ntrees + 1], gpair_off [groups + 1]; first, last, parent (uint32), length (float64), internal
    (uint8) per node; leaf_genome, leaf_species per leaf and leaf_class [3, leaves]; class_total per class; pair_a, pair_b per pair."""

    def __init__(self, ntrees, **arrays):
        self.ntrees = int(ntrees)
        for f, dt in _GENETREE_FIELDS:
            setattr(self, f, np.ascontiguousarray(arrays[f], dtype=dt).reshape(-1))
        self.nclasses, self.npairs, self.ngroups = int(self.class_off[-1]), int(self.gpair_off[-1]), int(self.group_off[-1])

    def args(self):
        """The ckm_genetree_args of these arrays (it borrows them: keep this object alive over the call)."""
        return GenetreeArgs(self.ntrees, *[getattr(self, f).ctypes.data if getattr(self, f).size else None for f, _ in _GENETREE_FIELDS])


def genetree_check(tables):
    """ckm_genetree_check: why the forest of a call would be refused, without a device.  Raises CkmError as genetree_run would."""
    a = tables.args()
    _chk(load().ckm_genetree_check(C.byref(a)))


def _genetree_call(entry, tables, budget_bytes):
    a = tables.args()
    _chk(load().ckm_genetree_check(C.byref(a)))               # (the output shapes below need offsets that are in order)
    o = dict(consistency=np.zeros(tables.nclasses), pair_flag=np.zeros(tables.npairs, dtype=np.uint8), group_node=np.zeros(tables.ngroups, dtype=np.uint32),
             group_mixed=np.zeros(tables.ngroups, dtype=np.uint8))
    info = GenetreeInfo()
    go = GenetreeOut(*[o[f].ctypes.data if o[f].size else None for f in ("consistency", "pair_flag", "group_node", "group_mixed")])
    _chk(entry(C.byref(a), int(budget_bytes), C.byref(go), C.byref(info)))
    o.update({f: int(getattr(info, f)) for f in ("nrounds", "ntrees", "launches")})
    o.update({f: getattr(info, f) for f in _GENETREE_MS})
    return o


def genetree_run(ctx, tables, budget_bytes=0):
    """The gene-tree tests of a packed forest (ckm_genetree_run).  Returns a dict: consistency [classes] float64, pair_flag [pairs] uint8,
    group_node [groups] uint32 (GENETREE_NONE: no flagged pair), group_mixed [groups] uint8; nrounds, ntrees, launches and the timings in ms."""
    L = load()
    return _genetree_call(lambda a, b, o, i: L.ckm_genetree_run(ctx.h, a, b, o, i), tables, budget_bytes)


def genetree_host(tables, budget_bytes=0):
    """The same call through the host executor (ckm_genetree_host): the same bits, no device.  For checks and comparisons; nothing in the
    package calls it in place of the device."""
    return _genetree_call(load().ckm_genetree_host, tables, budget_bytes)


NEARID_MAX_ROWS, NEARID_MAX_STRIDE, NEARID_MAX_TEXT_BYTES = 1 << 17, 1 << 24, 1 << 34


class NearidTables(object):
    """The arrays of one near-identity call as ckm_nearid_check / ckm_nearid_run take them (include/checkm_hip.h).  rows: a list of equally
    long bytes objects, or a [n_rows, row_len] uint8 array; they are copied into one uint8 array [n_rows, row_stride] whose stride is
    row_len rounded up to a multiple of 16, padded with 0.  limit: per row i, the pairs (i, j > i) are near iff they differ in fewer
    columns."""

    def __init__(self, rows, limit):
        if isinstance(rows, np.ndarray):
            body = np.ascontiguousarray(rows, dtype=np.uint8)
            body = body.reshape(body.shape[0], -1)
        else:
            rows = list(rows)
            body = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), len(rows[0]) if rows else 0)
        self.n_rows, self.row_len = int(body.shape[0]), int(body.shape[1])
        self.row_stride = max(16, (self.row_len + 15) // 16 * 16)
        self.text = np.zeros((self.n_rows, self.row_stride), dtype=np.uint8)
        self.text[:, :self.row_len] = body
        self.limit = np.ascontiguousarray(limit, dtype=np.uint32).reshape(-1)
        if self.limit.shape[0] != self.n_rows:
            raise ValueError("one limit per row")
        self.words = (self.n_rows + 63) // 64

    def args(self):
        """The ckm_nearid_args of these arrays (it borrows them: keep this object alive over the call)."""
        return NearidArgs(self.text.ctypes.data if self.text.size else None, self.n_rows, self.row_len, self.row_stride, self.limit.ctypes.data if self.limit.size else None)


def nearid_check(tables):
    """ckm_nearid_check: why a call would be refused, without a device.  Raises CkmError as nearid_run would."""
    a = tables.args()
    _chk(load().ckm_nearid_check(C.byref(a)))


def _nearid_call(entry, tables, budget_bytes):
    a = tables.args()
    _chk(load().ckm_nearid_check(C.byref(a)))                 # (the output shape below needs a call that is in range)
    o = dict(near=np.zeros((tables.n_rows, tables.words), dtype=np.uint64))
    info = NearidInfo()
    no = NearidOut(o["near"].ctypes.data)
    _chk(entry(C.byref(a), int(budget_bytes), C.byref(no), C.byref(info)))
    o.update({f: int(getattr(info, f)) for f in ("nbands", "npairs", "launches", "blocks")})
    o.update({f: getattr(info, f) for f in _NEARID_MS})
    return o


def nearid_run(ctx, tables, budget_bytes=0):
    """The near-identity pass (ckm_nearid_run).  Returns a dict: near [n_rows, ceil(n_rows / 64)] uint64, bit (j & 63) of word j // 64 of row
    i set iff j > i and rows i and j differ in fewer than limit[i] columns; nbands, npairs, launches, blocks and the timings in ms."""
    L = load()
    return _nearid_call(lambda a, b, o, i: L.ckm_nearid_run(ctx.h, a, b, o, i), tables, budget_bytes)


def nearid_host(tables, budget_bytes=0):
    """The same call through the host executor (ckm_nearid_host): the same bits, no device.  For checks and comparisons; nothing in the
    package calls it in place of the device."""
    return _nearid_call(load().ckm_nearid_host, tables, budget_bytes)
