# -*- coding: utf-8 -*-
"""ctypes binding of the C ABI in include/east_hip.h (libeast_hip.so).

Thin by design: numpy arrays in, numpy arrays out, every error code turned
into HipBackendError.  There is no CPU fallback -- if the library or a HIP
device is missing, every compute call raises.
"""
import atexit
import ctypes
import os

import numpy as np

from east import exceptions

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EAST_HIP_LIBRARY", os.path.join(_HERE, "_lib", "libeast_hip.so"))

_c_i64p = ctypes.POINTER(ctypes.c_int64)
_c_i32p = ctypes.POINTER(ctypes.c_int32)
_c_u32p = ctypes.POINTER(ctypes.c_uint32)
_c_u64p = ctypes.POINTER(ctypes.c_uint64)
_c_dblp = ctypes.POINTER(ctypes.c_double)

# name -> (restype, argtypes); mirrors include/east_hip.h one to one
SIGNATURES = {
    "east_hip_version": (ctypes.c_char_p, []),
    "east_hip_last_error": (ctypes.c_char_p, []),
    "east_hip_device_count": (ctypes.c_int, []),
    "east_hip_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p)]),
    "east_hip_reset": (ctypes.c_int, [ctypes.c_void_p]),
    "east_hip_destroy": (None, [ctypes.c_void_p]),
    "east_hip_build": (ctypes.c_int, [ctypes.c_void_p, _c_u32p, ctypes.c_int64, _c_i64p, _c_i32p, ctypes.c_int32]),
    "east_hip_build_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, _c_i64p, _c_i32p,
                                             ctypes.c_int32]),
    "east_hip_build_texts": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64, _c_i64p, ctypes.c_int32,
                                            ctypes.POINTER(ctypes.c_uint8), _c_u32p, _c_u32p, _c_u32p, _c_u32p,
                                            _c_u32p, ctypes.c_int32]),
    "east_hip_build_texts_v": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), _c_i64p, ctypes.c_int32,
                                              ctypes.POINTER(ctypes.c_uint8), _c_u32p, _c_u32p, _c_u32p, _c_u32p,
                                              _c_u32p, ctypes.c_int32]),
    "east_hip_get_prepared": (ctypes.c_int, [ctypes.c_void_p, _c_i64p, _c_i64p, _c_i32p, _c_u32p]),
    "east_hip_prepared_encoding": (ctypes.c_int, [ctypes.c_void_p]),
    "east_hip_set_symbol_encoding": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "east_hip_last_prep_ms": (ctypes.c_double, [ctypes.c_void_p]),
    "east_hip_get_tables": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32] + [_c_i32p] * 6),
    "east_hip_score_table": (ctypes.c_int, [ctypes.c_void_p, _c_u32p, _c_i64p, ctypes.c_int32, ctypes.c_int,
                                            _c_dblp, _c_dblp]),
    "east_hip_score_table_grouped": (ctypes.c_int, [ctypes.c_void_p, _c_u32p, _c_i64p, ctypes.c_int32, _c_i64p,
                                                    ctypes.c_int32, ctypes.c_int, _c_dblp]),
    "east_hip_get_lcp_intervals": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _c_i32p]),
    "east_hip_set_keyphrases": (ctypes.c_int, [ctypes.c_void_p, _c_u32p, _c_i64p, ctypes.c_int32]),
    "east_hip_score_resident": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "east_hip_score_probes": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_i64p]),
    "east_hip_score_resident_async": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "east_hip_synchronize": (ctypes.c_int, [ctypes.c_void_p]),
    "east_hip_stream": (ctypes.c_void_p, [ctypes.c_void_p]),
    "east_hip_build_info": (ctypes.c_int, [ctypes.c_void_p, _c_i64p, ctypes.c_int32]),
    "east_hip_last_build_ms": (ctypes.c_double, [ctypes.c_void_p]),
    "east_hip_last_score_ms": (ctypes.c_double, [ctypes.c_void_p]),
    "east_hip_debug_radix_sort_u64": (ctypes.c_int, [ctypes.c_int, _c_u64p, _c_u32p, ctypes.c_int64, ctypes.c_int]),
    "east_hip_debug_radix_sort_u32": (ctypes.c_int, [ctypes.c_int, _c_u32p, _c_u32p, ctypes.c_int64, ctypes.c_int]),
    "east_hip_debug_exclusive_scan": (ctypes.c_int, [ctypes.c_int, _c_u32p, _c_u32p, ctypes.c_int64]),
    "east_hip_debug_suffix_array": (ctypes.c_int, [ctypes.c_int, _c_u32p, ctypes.c_int64, ctypes.c_uint32, _c_i32p,
                                                   _c_i32p]),
    "east_hip_debug_suffix_array_ex": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32,
                                                      ctypes.c_uint32, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int32,
                                                      ctypes.c_int, _c_u32p, _c_u32p, _c_u32p, _c_i64p, _c_u32p]),
    "east_hip_plan_arena_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]),
    "east_hip_plan_arena_bytes_lean": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]),
    "east_hip_debug_set_rank_bucket_bytes": (ctypes.c_int, [ctypes.c_int64]),
    "east_hip_debug_set_window_sort": (ctypes.c_int, [ctypes.c_int]),
    "east_hip_debug_set_lds_rounds": (ctypes.c_int, [ctypes.c_int]),
    "east_hip_debug_set_persist": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "east_hip_debug_set_segmented_sort": (ctypes.c_int, [ctypes.c_int]),
    "east_hip_debug_set_speculation": (ctypes.c_int, [ctypes.c_int]),
    "east_hip_debug_set_eager_kgram": (ctypes.c_int, [ctypes.c_int]),
    "east_hip_debug_set_ann_wide_order": (ctypes.c_int, [ctypes.c_int]),
    "east_hip_debug_first_pass_hist": (ctypes.c_int, [ctypes.c_int, _c_u32p, ctypes.c_int64, _c_u32p, ctypes.c_int,
                                                      ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int,
                                                      ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint8), _c_u32p, _c_u32p,
                                                      _c_u32p, _c_u32p]),
    "east_hip_debug_annotate": (ctypes.c_int, [ctypes.c_int, _c_u32p, ctypes.c_int64, _c_i64p, ctypes.c_int32, _c_i32p,
                                               _c_u32p, _c_u32p, _c_u32p]),
    "east_hip_debug_child_tables": (ctypes.c_int, [ctypes.c_int, _c_u32p, ctypes.c_int64, _c_i64p, ctypes.c_int32, _c_i32p,
                                                   _c_u32p, _c_u32p, _c_u32p, _c_u32p, _c_u32p, _c_u32p]),
    "east_hip_debug_lcp": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32, _c_u32p,
                                          _c_i64p, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_u32p, ctypes.c_int, _c_u32p,
                                          _c_u32p, _c_u32p, _c_u32p, _c_u32p, _c_u32p]),
    "east_hip_debug_radix_sort_ex": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, _c_u32p, ctypes.c_int64,
                                                    ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_i64p, ctypes.c_int32, _c_u32p]),
    "east_hip_debug_radix_spine": (ctypes.c_int, [ctypes.c_int, _c_u32p, ctypes.c_int64, _c_u32p, _c_i64p, ctypes.c_int32,
                                                  _c_u32p, _c_u32p, _c_u32p]),
    "east_hip_debug_scan_ex": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _c_u32p, ctypes.c_int64, _c_u32p, _c_u32p]),
    "east_hip_debug_run_heads": (ctypes.c_int, [ctypes.c_int, _c_u64p, ctypes.c_int64, ctypes.c_int, _c_u32p, _c_u32p]),
    "east_hip_debug_scan_pair_bounded": (ctypes.c_int, [ctypes.c_int, _c_u32p, _c_u32p, ctypes.c_int64, ctypes.c_uint32,
                                                        ctypes.c_uint32, _c_u32p, _c_u32p]),
    "east_hip_debug_ascending_offsets": (ctypes.c_int, [ctypes.c_int, _c_u32p, ctypes.c_int64, ctypes.c_int64, _c_u32p]),
    "east_hip_debug_pyramid_level": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _c_u32p, ctypes.c_int64, _c_i64p]),
    "east_hip_debug_set_score_scratch": (ctypes.c_int, [ctypes.c_int64]),
    "east_hip_debug_set_score_path": (ctypes.c_int, [ctypes.c_int]),
    "east_hip_debug_set_score_grid": (ctypes.c_int, [ctypes.c_int64]),
    "east_hip_debug_set_text_stream": (ctypes.c_int, [ctypes.c_int64]),
    "east_hip_debug_set_text_ring": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64]),
    "east_hip_debug_alphabetic_code": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int32,
                                                      ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)]),
    "east_hip_debug_narrow_symbols": (ctypes.c_int, [_c_u32p, ctypes.c_int64, ctypes.POINTER(ctypes.c_uint16), ctypes.c_int]),
    "east_hip_debug_narrow_symbols8": (ctypes.c_int, [_c_u32p, ctypes.c_int64, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int]),
    "east_hip_group_create": (ctypes.c_int, [_c_i32p, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]),
    "east_hip_group_destroy": (None, [ctypes.c_void_p]),
    "east_hip_group_build": (ctypes.c_int, [ctypes.c_void_p, _c_u32p, ctypes.c_int64, _c_i64p, _c_i32p, ctypes.c_int32,
                                            ctypes.c_int32]),
    "east_hip_group_build_texts_v": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), _c_i64p, ctypes.c_int32,
                                                    ctypes.POINTER(ctypes.c_uint8), _c_u32p, _c_u32p, _c_u32p, _c_u32p,
                                                    _c_u32p, ctypes.c_int32]),
    "east_hip_group_shards": (ctypes.c_int, [ctypes.c_void_p, _c_i32p]),
    "east_hip_group_handle": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_int32]),
    "east_hip_score_table_multi": (ctypes.c_int, [ctypes.c_void_p, _c_u32p, _c_i64p, ctypes.c_int32, ctypes.c_int, _c_dblp]),
    "east_hip_group_info": (ctypes.c_int, [ctypes.c_void_p, _c_dblp, ctypes.c_int32]),
    "east_hip_debug_shard_documents": (ctypes.c_int, [_c_i64p, ctypes.c_int32, ctypes.c_int32, _c_i32p]),
    "east_hip_format_table_xml": (ctypes.c_int64, [_c_dblp, ctypes.c_int32, ctypes.c_int32, _c_i32p, _c_i32p,
                                                   ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_char_p),
                                                   ctypes.c_char_p, ctypes.c_int64]),
    "east_hip_format_table_csv": (ctypes.c_int64, [_c_dblp, ctypes.c_int32, ctypes.c_int32, _c_i32p, _c_i32p,
                                                   ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_char_p),
                                                   ctypes.c_char_p, ctypes.c_int64]),
    "east_hip_profile_enable": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "east_hip_profile_only": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p]),
    "east_hip_profile_report": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64]),
    "east_hip_cosine_build_texts": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64, _c_i64p, ctypes.c_int32,
                                                   ctypes.POINTER(ctypes.c_uint8), _c_u32p, _c_u32p, _c_u32p, _c_u32p,
                                                   _c_u32p, ctypes.c_int32, _c_u32p, _c_i64p, ctypes.c_int32]),
    "east_hip_cosine_build_texts_v": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), _c_i64p, ctypes.c_int32,
                                                     ctypes.POINTER(ctypes.c_uint8), _c_u32p, _c_u32p, _c_u32p, _c_u32p,
                                                     _c_u32p, ctypes.c_int32, _c_u32p, _c_i64p, ctypes.c_int32]),
    "east_hip_cosine_info": (ctypes.c_int, [ctypes.c_void_p, _c_i64p, ctypes.c_int32]),
    "east_hip_cosine_get_terms": (ctypes.c_int, [ctypes.c_void_p, _c_i64p, _c_u32p, _c_i64p]),
    "east_hip_cosine_set_classes": (ctypes.c_int, [ctypes.c_void_p, _c_i32p, ctypes.c_int32]),
    "east_hip_cosine_lookup": (ctypes.c_int, [ctypes.c_void_p, _c_u32p, _c_i64p, ctypes.c_int32, _c_i32p]),
    "east_hip_cosine_score_table": (ctypes.c_int, [ctypes.c_void_p, _c_i32p, _c_i64p, ctypes.c_int64, ctypes.c_int32,
                                                   ctypes.c_int32, _c_dblp]),
    "east_hip_debug_set_term_hash_bits": (ctypes.c_int, [ctypes.c_int]),
    "east_hip_bm25_score_table": (ctypes.c_int, [ctypes.c_void_p, _c_i32p, _c_i64p, ctypes.c_int64, ctypes.c_int32,
                                                 ctypes.c_double, ctypes.c_double, _c_dblp]),
    "east_hip_bm25_info": (ctypes.c_int, [ctypes.c_void_p, _c_dblp, ctypes.c_int32]),
    "east_hip_debug_set_bm25_strip": (ctypes.c_int, [ctypes.c_int32]),
    "east_hip_graph_build_resident": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _c_i32p, ctypes.c_int64, ctypes.c_double,
                                                     ctypes.c_double, ctypes.c_double, _c_i64p]),
    "east_hip_graph_build_host": (ctypes.c_int, [ctypes.c_void_p, _c_dblp, ctypes.c_int32, ctypes.c_int32, _c_i32p,
                                                 ctypes.c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_double, _c_i64p]),
    "east_hip_graph_fetch": (ctypes.c_int, [ctypes.c_void_p] + [_c_i32p] * 5),
    "east_hip_last_graph_ms": (ctypes.c_double, [ctypes.c_void_p]),
    "east_hip_synonyms_build": (ctypes.c_int, [ctypes.c_void_p, _c_i32p, _c_i32p, _c_i32p, ctypes.c_int64, _c_i32p,
                                               ctypes.c_int32, ctypes.c_int32]),
    "east_hip_synonyms_info": (ctypes.c_int, [ctypes.c_void_p, _c_i64p, ctypes.c_int32]),
    "east_hip_synonyms_get_rows": (ctypes.c_int, [ctypes.c_void_p, _c_i64p, _c_i32p, _c_i32p, _c_dblp, _c_dblp]),
    "east_hip_synonyms_similarity": (ctypes.c_int, [ctypes.c_void_p, _c_i32p, _c_i32p, ctypes.c_int64, _c_dblp]),
    "east_hip_synonyms_pairs": (ctypes.c_int, [ctypes.c_void_p, _c_i32p, ctypes.c_int32, ctypes.c_double, _c_i64p]),
    "east_hip_synonyms_fetch": (ctypes.c_int, [ctypes.c_void_p, _c_i32p, _c_i32p, _c_dblp]),
    "east_hip_last_synonyms_ms": (ctypes.c_double, [ctypes.c_void_p]),
    "east_hip_debug_set_synonyms_chunk": (ctypes.c_int, [ctypes.c_int]),
    "east_hip_top_build_resident": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                   ctypes.c_double, _c_i64p]),
    "east_hip_top_build_host": (ctypes.c_int, [ctypes.c_void_p, _c_dblp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                               ctypes.c_int32, ctypes.c_double, _c_i64p]),
    "east_hip_top_fetch": (ctypes.c_int, [ctypes.c_void_p, _c_i32p, _c_i32p, _c_dblp]),
    "east_hip_last_top_ms": (ctypes.c_double, [ctypes.c_void_p]),
    "east_hip_debug_set_top_tile": (ctypes.c_int, [ctypes.c_int]),
    "east_hip_similarity_build_resident": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, _c_i64p]),
    "east_hip_similarity_build_host": (ctypes.c_int, [ctypes.c_void_p, _c_dblp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                      _c_i64p]),
    "east_hip_similarity_fetch": (ctypes.c_int, [ctypes.c_void_p, _c_dblp, _c_dblp]),
    "east_hip_last_similarity_ms": (ctypes.c_double, [ctypes.c_void_p]),
    "east_hip_related_build": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, _c_i64p]),
    "east_hip_related_fetch": (ctypes.c_int, [ctypes.c_void_p, _c_dblp, _c_dblp, _c_i32p]),
    "east_hip_last_related_ms": (ctypes.c_double, [ctypes.c_void_p]),
    "east_hip_debug_set_related_chunk": (ctypes.c_int, [ctypes.c_int64]),
    "east_hip_text_similarity_build": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _c_i64p]),
    "east_hip_text_similarity_fetch": (ctypes.c_int, [ctypes.c_void_p, _c_dblp, _c_dblp, _c_i32p]),
    "east_hip_last_text_similarity_ms": (ctypes.c_double, [ctypes.c_void_p]),
    "east_hip_debug_set_text_similarity_batch": (ctypes.c_int, [ctypes.c_int64]),
    "east_hip_clusters_build_resident": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _c_i64p]),
    "east_hip_clusters_build_host": (ctypes.c_int, [ctypes.c_void_p, _c_dblp, ctypes.c_int32, _c_i64p]),
    "east_hip_clusters_build_resident_linkage": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, _c_i64p]),
    "east_hip_clusters_build_host_linkage": (ctypes.c_int, [ctypes.c_void_p, _c_dblp, ctypes.c_int32, ctypes.c_int32, ctypes.c_double,
                                             _c_i64p]),
    "east_hip_clusters_fetch": (ctypes.c_int, [ctypes.c_void_p, _c_i32p, _c_i32p, _c_dblp]),
    "east_hip_clusters_cut_threshold": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, _c_i32p, _c_i64p]),
    "east_hip_clusters_cut_count": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _c_i32p, _c_i64p]),
    "east_hip_last_clusters_ms": (ctypes.c_double, [ctypes.c_void_p]),
    "east_hip_phrases_build": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                              ctypes.c_int64, _c_i64p]),
    "east_hip_phrases_fetch": (ctypes.c_int, [ctypes.c_void_p, _c_i32p, _c_i32p, _c_i32p, _c_i32p, _c_i32p, _c_i32p, _c_i64p,
                                              _c_u32p]),
    "east_hip_phrases_levels": (ctypes.c_int, [ctypes.c_void_p, _c_i64p, _c_i64p]),
    "east_hip_last_phrases_ms": (ctypes.c_double, [ctypes.c_void_p]),
    "east_hip_terms_build": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _c_i32p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                            _c_i64p]),
    "east_hip_terms_fetch": (ctypes.c_int, [ctypes.c_void_p, _c_i32p, _c_i32p, _c_i32p, _c_dblp, _c_i32p, _c_i32p]),
    "east_hip_terms_fetch_vectors": (ctypes.c_int, [ctypes.c_void_p, _c_i64p, _c_i32p, _c_dblp, _c_i32p]),
    "east_hip_last_terms_ms": (ctypes.c_double, [ctypes.c_void_p]),
    "east_hip_debug_set_terms_select": (ctypes.c_int, [ctypes.c_int]),
    "east_hip_overlap_build": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, _c_i64p]),
    "east_hip_overlap_fetch": (ctypes.c_int, [ctypes.c_void_p, _c_dblp, _c_dblp, _c_i32p]),
    "east_hip_last_overlap_ms": (ctypes.c_double, [ctypes.c_void_p]),
    "east_hip_debug_set_overlap_route": (ctypes.c_int, [ctypes.c_int]),
    "east_hip_debug_set_overlap_batch": (ctypes.c_int, [ctypes.c_int64]),
    "east_hip_passages_build": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _c_i32p, _c_i32p,
                                               ctypes.c_int64, _c_i64p]),
    "east_hip_passages_fetch": (ctypes.c_int, [ctypes.c_void_p, _c_i64p, _c_i32p, _c_i32p, _c_i32p, _c_i32p, _c_i32p, _c_i32p, _c_i32p]),
    "east_hip_passages_phases": (ctypes.c_int, [ctypes.c_void_p, _c_dblp]),
    "east_hip_last_passages_ms": (ctypes.c_double, [ctypes.c_void_p]),
    "east_hip_debug_set_passages_route": (ctypes.c_int, [ctypes.c_int]),
}

BUILD_INFO_FIELDS = ("n_total", "n_docs", "n_strings", "sigma_text", "bits_level0", "dc3_levels", "arena_bytes",
                     "arena_high_water", "radix_passes", "radix_elements", "radix_element_bytes",
                     "radix_passes_u32", "radix_elements_u32", "radix_passes_u64", "radix_elements_u64",
                     "dc3_levels_resolved", "merge_elements", "refine_rounds", "window_sorted", "lds_sorted",
                     "fused_finish", "first_kept", "first_n", "ht_keys", "seg_sort", "narrow_upload", "persist_rounds",
                     "first_hist_fused", "ann_wide_order", "kgram_queued", "ann_listed")
COSINE_INFO_FIELDS = ("built", "n_docs", "kept_tokens", "words", "terms", "classes", "postings", "hash_attempts", "build_us",
                      "score_us")
BM25_INFO_FIELDS = ("N", "avgdl", "k1", "b", "weights_computed")        # east_hip_bm25_info (k1, b: NaN while no weights are cached)

GRAPH_SOURCE_AST, GRAPH_SOURCE_COSINE, GRAPH_SOURCE_UPLOADED = 0, 1, 2      # east_hip_graph_build_resident: which resident table
GRAPH_SOURCE_SIMILARITY = 3                 # east_hip_top_build_resident only: the matrix the last similarity build left
GRAPH_SOURCE_RELATED = 4                    # east_hip_top_build_resident only: the matrix the last related build left
GRAPH_SOURCE_COSINE_TEXTS = 5               # east_hip_top_build_resident only: the matrix the last cosine texts build left
COSINE_TEXTS_CHUNK, COSINE_TEXTS_SEG = 32, 8192      # csrc/cosine_texts.h: the units of a staged chunk and of a segment (texts_build reports them)
COSINE_TEXTS_INFO_FIELDS = ("n_docs", "units", "postings", "tiles", "segments", "launches", "chunk_units", "segment_units")
GRAPH_SOURCE_OVERLAP = 6                    # the ranking and the clusters: the matrix the last shingle overlap build left
OVERLAP_DIRECTED, OVERLAP_SYMMETRIC = 0, 1  # EAST_HIP_OVERLAP_*
OVERLAP_ORIENTATIONS = ("directed", "symmetric")
OVERLAP_INFO_FIELDS = ("n_docs", "kept_tokens", "shingle_positions", "distinct_shingles", "shared_shingles", "postings", "segments",
                       "launches", "route", "levels", "tiles", "words", "operands_us", "product_us")          # east_hip_overlap_build: out
PASSAGES_INFO_FIELDS = ("n_docs", "kept_tokens", "pairs", "shared_shingles", "postings", "bit_words", "shared_starts", "passages",
                        "returned", "launches", "route", "levels")                                            # east_hip_passages_build: out
TERMS_INFO_FIELDS = ("n_docs", "groups", "units", "postings", "entries", "passing", "sorted", "radix_passes", "launches",
                     "grouping_sort_skipped")                           # east_hip_terms_build: out
CLUSTERS_INFO_FIELDS = ("members", "merges", "rounds", "launches")      # east_hip_clusters_build_*: out
LINKAGE_SINGLE, LINKAGE_COMPLETE, LINKAGE_AVERAGE = 0, 1, 2            # EAST_HIP_LINKAGE_*
LINKAGES = {"single": LINKAGE_SINGLE, "complete": LINKAGE_COMPLETE, "average": LINKAGE_AVERAGE}
RELATED_DIRECTED, RELATED_SYMMETRIC = 0, 1                               # east_hip_related_build: the orientation
DEBUG_GUARD = 4096                          # east_hip_debug_radix_sort_ex and its kin: elements behind every output
SCAN_EXCLUSIVE, SCAN_INCLUSIVE, SCAN_EXCLUSIVE_IN_PLACE, SCAN_INCLUSIVE_IN_PLACE, SCAN_WITH_TOTAL = range(5)    # east_hip_debug_scan_ex
TOP_BY_TEXT, TOP_BY_KEYPHRASE = 0, 1                                     # east_hip_top_build_*: what a segment is
TOP_MAX_N = 1024

_lib = None


def load():
    """Load libeast_hip.so (built by __graft_entry__.build() / csrc/Makefile)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise exceptions.HipBackendError(
                reason="%s not found -- build it with `make -C ast-text-analysis_amd/csrc` "
                       "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback" % LIB_PATH)
        try:
            lib = ctypes.CDLL(LIB_PATH)
        except OSError as e:
            raise exceptions.HipBackendError(reason="cannot load %s: %s" % (LIB_PATH, e))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _linkage_arguments(linkage, floor):
    """(the EAST_HIP_LINKAGE_* value of a name or of a value, the floor as a double: NaN = none)"""
    if isinstance(linkage, str):
        if linkage not in LINKAGES:
            raise exceptions.HipBackendError(reason="unknown linkage %r: one of 'single', 'complete', 'average'" % (linkage,))
        linkage = LINKAGES[linkage]
    return int(linkage), float("nan") if floor is None else float(floor)


def _check(rc):
    if rc != 0:
        msg = load().east_hip_last_error()
        raise exceptions.HipBackendError(reason="%s (code %d)" % (msg.decode("utf-8", "replace") if msg else "?", rc))


def _ptr(a, t):
    return a.ctypes.data_as(t)


def device_count():
    c = load().east_hip_device_count()
    return c if c > 0 else 0


def default_device():
    for var in ("EAST_HIP_DEVICE", "LOCAL_RANK"):
        if os.environ.get(var, "") != "":
            return int(os.environ[var])
    return 0


_unicode_tables = None


def unicode_tables():
    """The interpreter's own Unicode data for east_hip_build_texts: per code point below U+0A00 the
    class (bit 0: matches [\\w'] under re.U, i.e. str.isalnum() or '_' or "'"; bit 1: str.isdigit())
    and the 1:1 upper-case mapping; a bitmap of the word characters from U+0A00 up."""
    global _unicode_tables
    if _unicode_tables is None:
        lim = 0x0A00
        cls = np.zeros(lim, dtype=np.uint8)
        upper = np.arange(lim, dtype=np.uint32)
        for cp in range(lim):
            ch = chr(cp)
            cls[cp] = (1 if (ch.isalnum() or ch in "_'") else 0) | (2 if ch.isdigit() else 0)
            up = ch.upper()
            if len(up) == 1:
                upper[cp] = ord(up)
        n_hi = 0x110000 - lim
        wbits = np.zeros(n_hi, dtype=np.uint8)
        dbits = np.zeros(n_hi, dtype=np.uint8)
        hi_from, hi_to = [], []
        for cp in range(lim, 0x110000):
            ch = chr(cp)
            if ch.isalnum():
                wbits[cp - lim] = 1
                if ch.isdigit():
                    dbits[cp - lim] = 1
            up = ch.upper()
            if len(up) == 1 and up != ch:
                hi_from.append(cp)
                hi_to.append(ord(up))
        word_hi = np.packbits(wbits, bitorder="little").view(np.uint32).copy()
        digit_hi = np.packbits(dbits, bitorder="little").view(np.uint32).copy()
        _unicode_tables = (cls, upper, word_hi, digit_hi, np.array(hi_from, dtype=np.uint32),
                           np.array(hi_to, dtype=np.uint32))
    return _unicode_tables


JOIN_FREE_MAX_TEXTS = 512               # build_texts: up to this many texts of at least ...
JOIN_FREE_MIN_BYTES = 1 << 20           # ... this many bytes in all go to the device one by one, unjoined,
JOIN_FREE_RING_BYTES = 8 << 20          # ... and any number of texts from this size on (the streamed preparation: the
#                                         library copies them into a pinned ring with a few threads; joining 256 MB in
#                                         Python takes 50 ms, four times what the device needs for the whole index)
JOIN_FREE_RING_MIN_MEAN = 4096          # ... while a text averages this many bytes
JOIN_FREE_RING_MAX_TEXTS = 1 << 20
POOL_HANDLES = 2                        # recycled handles kept per device ...
POOL_MAX_ARENA_BYTES = 256 << 20        # ... if their device arena is at most this large
_handle_pool = {}


def _drain_pool():
    lib = _lib
    for handles in _handle_pool.values():
        while handles:
            if lib is not None:
                lib.east_hip_destroy(handles.pop())
            else:
                handles.pop()


atexit.register(_drain_pool)


def _raw_texts(texts):
    return [t if isinstance(t, bytes) else t.encode("utf-8", errors="surrogatepass") for t in texts]


def _table_args():
    """unicode_tables() as the arguments of east_hip_build_texts[_v] / east_hip_cosine_build_texts[_v]."""
    cls, upper, word_hi, digit_hi, hi_from, hi_to = unicode_tables()
    return (_ptr(cls, ctypes.POINTER(ctypes.c_uint8)), _ptr(upper, _c_u32p), _ptr(word_hi, _c_u32p),
            _ptr(digit_hi, _c_u32p), _ptr(hi_from, _c_u32p), _ptr(hi_to, _c_u32p), hi_from.size)


def _join_free(raw):
    """Whether texts go to the device one by one (the _v entry points) rather than joined into one blob."""
    total = sum(len(t) for t in raw)
    # (... through the pinned ring only while a text averages JOIN_FREE_RING_MIN_MEAN bytes: half a million one-line
    # texts cost more as a ctypes pointer array than the one b"".join they would save)
    return (len(raw) <= JOIN_FREE_MAX_TEXTS and total >= JOIN_FREE_MIN_BYTES) or \
        (len(raw) <= JOIN_FREE_RING_MAX_TEXTS and total >= JOIN_FREE_RING_BYTES and total >= JOIN_FREE_RING_MIN_MEAN * len(raw))


def _separate(raw):
    """The texts where they lie, for the _v entry points: (pointer array, lengths int64).  The pointers borrow from `raw`."""
    return (ctypes.c_char_p * len(raw))(*raw), np.array([len(t) for t in raw], dtype=np.int64)


def _joined(raw):
    """Every text followed by one 0xFF, in a single copy, and the D + 1 offsets."""
    blob = b"\xff".join(raw + [b""])
    offsets = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum([len(t) + 1 for t in raw], out=offsets[1:])
    return blob, offsets


class GraphArrays(object):
    """A keyphrase graph as the device built it (include/east_hip.h, "The keyphrase graph"): `support` per node position,
    `kept` = the node positions in order, and per edge -- in the order of applications.py:111-141 -- `edge_source`,
    `edge_target` (positions) and `edge_shared` (texts that hold both); all int32."""

    __slots__ = ("support", "kept", "edge_source", "edge_target", "edge_shared")

    def __init__(self, support, kept, edge_source, edge_target, edge_shared):
        self.support, self.kept = support, kept
        self.edge_source, self.edge_target, self.edge_shared = edge_source, edge_target, edge_shared


def _table_build(resident, host, h, source, table, noun, *args):
    """One *_build_resident / *_build_host pair: resident(h, source, *args) when table is None, else host(h, table, K, D,
    *args) of the K x D host array `table`; noun names the consumer where the array is refused."""
    if table is None:
        _check(resident(h, int(source), *args))
        return
    table = np.ascontiguousarray(table, dtype=np.float64)
    if table.ndim != 2:
        raise exceptions.HipBackendError(reason="the score table of %s is a K x D array" % noun)
    _check(host(h, _ptr(table, _c_dblp), table.shape[0], table.shape[1], *args))


def _graph_build(lib, h, source, table, rows, relevance_threshold, support_threshold, referral_confidence):
    """east_hip_graph_build_resident (table None) / _host, then east_hip_graph_fetch."""
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    counts = np.zeros(2, dtype=np.int64)
    _table_build(lib.east_hip_graph_build_resident, lib.east_hip_graph_build_host, h, source, table, "a keyphrase graph",
                 _ptr(rows, _c_i32p), rows.size, float(relevance_threshold), float(support_threshold),
                 float(referral_confidence), _ptr(counts, _c_i64p))
    out = GraphArrays(np.empty(rows.size, dtype=np.int32), np.empty(int(counts[0]), dtype=np.int32),
                      *(np.empty(int(counts[1]), dtype=np.int32) for _ in range(3)))
    _check(lib.east_hip_graph_fetch(h, *(_ptr(getattr(out, name), _c_i32p) for name in GraphArrays.__slots__)))
    return out


class TopArrays(object):
    """A ranking as the device selected it (include/east_hip.h, "Ranked keyphrases"): `count[S]` (int32), and per segment
    its best members first: `index[S, n]` (int32, -1 behind count[s]) and `score[S, n]` (float64, the table's own bytes,
    0.0 behind count[s])."""

    __slots__ = ("count", "index", "score")

    def __init__(self, count, index, score):
        self.count, self.index, self.score = count, index, score


def _top_build(lib, h, source, table, axis, n, threshold):
    """east_hip_top_build_resident (table None) / _host, then east_hip_top_fetch."""
    out = np.zeros(2, dtype=np.int64)
    _table_build(lib.east_hip_top_build_resident, lib.east_hip_top_build_host, h, source, table, "a ranking", int(axis),
                 int(n), float(threshold), _ptr(out, _c_i64p))
    S = int(out[0])
    found = TopArrays(np.empty(S, dtype=np.int32), np.empty((S, int(n)), dtype=np.int32), np.empty((S, int(n)), dtype=np.float64))
    _check(lib.east_hip_top_fetch(h, _ptr(found.count, _c_i32p), _ptr(found.index, _c_i32p), _ptr(found.score, _c_dblp)))
    return found


def _similarity_build(lib, h, source, table, axis):
    """east_hip_similarity_build_resident (table None) / _host -> (M, L)."""
    out = np.zeros(2, dtype=np.int64)
    _table_build(lib.east_hip_similarity_build_resident, lib.east_hip_similarity_build_host, h, source, table,
                 "a similarity matrix", int(axis), _ptr(out, _c_i64p))
    return int(out[0]), int(out[1])


def _matrix_fetch(fetch, h, M, count=True):
    """The fetch entry point of an M x M matrix consumer -> (matrix[M, M], a double a member[M]) and, where the consumer
    counts (count=True), an int32 a member[M]."""
    found = (np.empty((M, M), dtype=np.float64), np.empty(M, dtype=np.float64)) + ((np.empty(M, dtype=np.int32),) if count else ())
    _check(fetch(h, *(_ptr(x, _c_i32p if x.dtype == np.int32 else _c_dblp) for x in found)))
    return found


PHRASES_MAX_WORDS = 8                       # csrc/phrases.h: PHR_MAX_WORDS


class TermArrays(object):
    """Characteristic terms as arrays (include/east_hip.h, "Characteristic terms"): members[G] the texts of every group,
    count[G] its listed terms, and per place [G, n] the unit (a term or a class of the vector space), its value, the group's
    texts that hold it and its texts in the whole collection; places behind count[g] hold -1 and NaN.  info: the build's
    out as {TERMS_INFO_FIELDS: value}."""

    __slots__ = ("members", "count", "unit", "value", "texts", "df", "info")

    def __init__(self, members, count, unit, value, texts, df, info=None):
        self.members, self.count, self.unit, self.value, self.texts, self.df, self.info = members, count, unit, value, texts, df, info


class PassageArrays(object):
    """Shared passages as the device left them (include/east_hip.h, "Shared passages"): per pair `starts`, `covered`, `found`
    (int32[pairs]) and `pair_off` (int64[pairs + 1]); per returned passage `start`, `words`, `at` (int32[pair_off[-1]],
    collection positions, pair by pair, longest first); `text_start` (int32[D + 1]); `info` = {PASSAGES_INFO_FIELDS: value}."""
    __slots__ = ("pair_off", "starts", "covered", "found", "start", "words", "at", "text_start", "info")


def _passages(lib, h, pairs_a, pairs_b, words, min_words, per_pair):
    pa, pb = np.ascontiguousarray(pairs_a, dtype=np.int32), np.ascontiguousarray(pairs_b, dtype=np.int32)
    if pa.ndim != 1 or pa.shape != pb.shape:
        raise ValueError("passages: pairs_a and pairs_b must be two lists of one length")
    out = np.zeros(len(PASSAGES_INFO_FIELDS), dtype=np.int64)
    _check(lib.east_hip_passages_build(h, int(words), int(min_words), int(per_pair), _ptr(pa, _c_i32p), _ptr(pb, _c_i32p), pa.size,
                                       _ptr(out, _c_i64p)))
    found = PassageArrays()
    found.info = dict(zip(PASSAGES_INFO_FIELDS, (int(x) for x in out)))
    n, R, D = pa.size, int(out[8]), int(out[0])
    found.pair_off = np.zeros(n + 1, dtype=np.int64)
    found.starts, found.covered, found.found = (np.zeros(n, dtype=np.int32) for _ in range(3))
    found.start, found.words, found.at = (np.zeros(R, dtype=np.int32) for _ in range(3))
    found.text_start = np.zeros(D + 1, dtype=np.int32)
    _check(lib.east_hip_passages_fetch(h, _ptr(found.pair_off, _c_i64p), *[_ptr(x, _c_i32p) for x in (
        found.starts, found.covered, found.found, found.start, found.words, found.at, found.text_start)]))
    return found


class PhraseArrays(object):
    """Extracted phrases as the device left them (include/east_hip.h, "Phrase extraction"), best first: per phrase `words`,
    `count`, `texts`, `first`, `first_text` (int32[returned]); `term_ids` (int32, ragged by the prefix sum of words);
    `text_off` (int64[returned + 1]) and `text` (uint32 code points, the words joined by one space); `candidates` = the
    candidates before the cut by N; `levels`, `domain[8]`, `survivors[8]` = what the levels did."""
    __slots__ = ("words", "count", "texts", "first", "first_text", "term_ids", "text_off", "text", "candidates", "levels",
                 "domain", "survivors")

    def strings(self):
        """The phrases' text as a list of str."""
        whole = self.text.astype("<u4").tobytes().decode("utf-32-le", errors="surrogatepass")
        return [whole[a:e] for a, e in zip(self.text_off[:-1].tolist(), self.text_off[1:].tolist())]


def _phrases(lib, h, n, max_words, min_words, min_count, min_texts):
    out = np.zeros(4, dtype=np.int64)
    _check(lib.east_hip_phrases_build(h, int(min_words), int(max_words), int(min_count), int(min_texts), int(n),
                                      _ptr(out, _c_i64p)))
    R = int(out[0])
    found = PhraseArrays()
    rows = [np.zeros(R, dtype=np.int32) for _ in range(5)]
    found.words, found.count, found.texts, found.first, found.first_text = rows
    found.text_off = np.zeros(R + 1, dtype=np.int64)
    found.text = np.zeros(int(out[2]), dtype=np.uint32)
    found.domain, found.survivors = np.zeros(PHRASES_MAX_WORDS, dtype=np.int64), np.zeros(PHRASES_MAX_WORDS, dtype=np.int64)
    # (the ids are as many as the words of the returned phrases: the rows first)
    _check(lib.east_hip_phrases_fetch(h, *([_ptr(r, _c_i32p) for r in rows] + [None, _ptr(found.text_off, _c_i64p),
                                                                                _ptr(found.text, _c_u32p)])))
    found.term_ids = np.zeros(int(found.words.sum()), dtype=np.int32)
    _check(lib.east_hip_phrases_fetch(h, None, None, None, None, None, _ptr(found.term_ids, _c_i32p), None, None))
    _check(lib.east_hip_phrases_levels(h, _ptr(found.domain, _c_i64p), _ptr(found.survivors, _c_i64p)))
    found.candidates, found.levels = int(out[1]), int(out[3])
    return found


class _ResidentTableConsumers(object):
    """The graph, the ranking and the similarity of the score table that lies on the device of a handle (self._lib,
    self._h): the table `_table_source` names -- the AST table of a HipIndex, the cosine table of a HipCosineIndex."""

    _table_source = None
    _sim_M = _rel_M = _texts_M = 0      # the members of the handle's last similarity / relatedness / text cosine matrix (0: none yet)

    @property
    def _sim_holder(self):
        """The HipIndex that remembers the size of the handle's last similarity matrix."""
        return self

    # -- phrase extraction -----------------------------------------------------
    def phrases(self, n=0, max_words=3, min_words=1, min_count=2, min_texts=1):
        """The repeated phrases of the texts the handle's cosine term index holds (include/east_hip.h, "Phrase
        extraction"), best first; n = 0: every candidate -> PhraseArrays."""
        return _phrases(self._lib, self._h, n, max_words, min_words, min_count, min_texts)

    @property
    def last_phrases_ms(self):
        return float(self._lib.east_hip_last_phrases_ms(self._h))

    # -- keyphrase graph -------------------------------------------------------
    def graph(self, rows, relevance_threshold, support_threshold, referral_confidence):
        """The keyphrase graph of the score table the last score call left on the device (rows[p] = the table row of node
        position p) -> GraphArrays."""
        return _graph_build(self._lib, self._h, self._table_source, None, rows, relevance_threshold, support_threshold,
                            referral_confidence)

    @property
    def last_graph_ms(self):
        return float(self._lib.east_hip_last_graph_ms(self._h))

    # -- ranked keyphrases -----------------------------------------------------
    def top(self, axis, n, threshold=-np.inf):
        """The n best members of every segment of the score table the last score call left on the device (axis
        TOP_BY_TEXT: per text its keyphrases, TOP_BY_KEYPHRASE: per keyphrase its texts) -> TopArrays."""
        return _top_build(self._lib, self._h, self._table_source, None, axis, n, threshold)

    @property
    def last_top_ms(self):
        return float(self._lib.east_hip_last_top_ms(self._h))

    # -- similar texts and keyphrases --------------------------------------------
    def _similarity(self, source, table, axis):
        self._sim_holder._sim_M, L = _similarity_build(self._lib, self._h, source, table, axis)
        return self._sim_holder._sim_M, L

    def similarity(self, axis):
        """The cosine of every two profiles of the score table the last score call left on the device (axis TOP_BY_TEXT:
        the texts' columns, TOP_BY_KEYPHRASE: the keyphrases' rows); the M x M matrix stays on the device -> (M, L)."""
        return self._similarity(self._table_source, None, axis)

    def similarity_matrix(self):
        """The last similarity matrix of this handle and the squared norms of its profiles -> (matrix[M, M], norm2[M])."""
        return _matrix_fetch(self._lib.east_hip_similarity_fetch, self._h, self._sim_holder._sim_M, count=False)

    def similar(self, axis, n, threshold=-np.inf):
        """similarity(axis), then the n most similar other members of every member (the ranking of the matrix by row: the
        NaN on its diagonal is never eligible) -> TopArrays.  It is the handle's one ranking: it replaces top()'s."""
        self.similarity(axis)
        return self.rank_similarity(n, threshold)

    def rank_similarity(self, n, threshold=-np.inf):
        """Another ranking of the last similarity matrix (other n, other threshold): no new matrix."""
        return _top_build(self._lib, self._h, GRAPH_SOURCE_SIMILARITY, None, TOP_BY_KEYPHRASE, n, threshold)

    @property
    def last_similarity_ms(self):
        return float(self._lib.east_hip_last_similarity_ms(self._h))

    # -- clusters ----------------------------------------------------------------
    def _clusters_built(self, out):
        info = dict(zip(CLUSTERS_INFO_FIELDS, (int(x) for x in out)))
        self._sim_holder._clu_info = info
        return info

    def clusters_build(self, source, linkage="single", floor=None):
        """Clusters (include/east_hip.h, "Clusters") of a square matrix that lies on the device of this handle:
        GRAPH_SOURCE_SIMILARITY, GRAPH_SOURCE_RELATED (symmetric), GRAPH_SOURCE_COSINE_TEXTS, or GRAPH_SOURCE_UPLOADED = the
        copy the last clusters_build_host left.  linkage: "single", "complete", "average" or an EAST_HIP_LINKAGE_* value;
        floor: only merges of at least this similarity are made (None: all) -> {CLUSTERS_INFO_FIELDS: value}."""
        out = np.zeros(len(CLUSTERS_INFO_FIELDS), dtype=np.int64)
        linkage, floor = _linkage_arguments(linkage, floor)
        if linkage == LINKAGE_SINGLE and floor != floor:
            _check(self._lib.east_hip_clusters_build_resident(self._h, int(source), _ptr(out, _c_i64p)))
        else:
            _check(self._lib.east_hip_clusters_build_resident_linkage(self._h, int(source), linkage, floor, _ptr(out, _c_i64p)))
        return self._clusters_built(out)

    def clusters_build_host(self, matrix, linkage="single", floor=None):
        """The same of an M x M host array, which is uploaded and checked for symmetry first."""
        matrix = np.ascontiguousarray(matrix, dtype=np.float64)
        if matrix.ndim != 2 or matrix.shape[0] != matrix.shape[1]:
            raise exceptions.HipBackendError(reason="the matrix of clusters is an M x M array")
        out = np.zeros(len(CLUSTERS_INFO_FIELDS), dtype=np.int64)
        linkage, floor = _linkage_arguments(linkage, floor)
        pointer = _ptr(matrix, _c_dblp) if matrix.size else None
        if linkage == LINKAGE_SINGLE and floor != floor:
            _check(self._lib.east_hip_clusters_build_host(self._h, pointer, matrix.shape[0], _ptr(out, _c_i64p)))
        else:
            _check(self._lib.east_hip_clusters_build_host_linkage(self._h, pointer, matrix.shape[0], linkage, floor, _ptr(out, _c_i64p)))
        return self._clusters_built(out)

    def clusters_merges(self):
        """The dendrogram of the last clusters build, strongest merge first -> (merge_a int32, merge_b int32, merge_w
        float64: the matrix's own bytes of S[a][b], a < b)."""
        info = getattr(self._sim_holder, "_clu_info", None) or {"merges": 0}
        F = info["merges"]
        a, b, w = np.empty(F, dtype=np.int32), np.empty(F, dtype=np.int32), np.empty(F, dtype=np.float64)
        _check(self._lib.east_hip_clusters_fetch(self._h, _ptr(a, _c_i32p), _ptr(b, _c_i32p), _ptr(w, _c_dblp)))
        return a, b, w

    def clusters_cut(self, threshold=None, k=None):
        """Flat clusters of the last build: the merges with similarity >= threshold, or the first merges that leave k
        clusters (exactly one of the two) -> (labels int32: the smallest member of every member's cluster, clusters,
        merges applied)."""
        if (threshold is None) == (k is None):
            raise exceptions.HipBackendError(reason="a cut of clusters takes a threshold or a number of clusters, one of the two")
        info = getattr(self._sim_holder, "_clu_info", None) or {"members": 0}
        labels, out = np.empty(info["members"], dtype=np.int32), np.zeros(2, dtype=np.int64)
        if threshold is not None:
            _check(self._lib.east_hip_clusters_cut_threshold(self._h, float(threshold), _ptr(labels, _c_i32p), _ptr(out, _c_i64p)))
        else:
            _check(self._lib.east_hip_clusters_cut_count(self._h, int(k), _ptr(labels, _c_i32p), _ptr(out, _c_i64p)))
        return labels, int(out[0]), int(out[1])

    @property
    def last_clusters_ms(self):
        return float(self._lib.east_hip_last_clusters_ms(self._h))


class HipIndex(_ResidentTableConsumers):
    """One device-resident batch of annotated suffix arrays (an AST shard)."""

    _table_source = GRAPH_SOURCE_AST

    def __init__(self, device=None, reserve_symbols=0):
        self._lib = load()
        self._h = ctypes.c_void_p()
        self.device = default_device() if device is None else int(device)
        pooled = _handle_pool.get(self.device)
        if pooled and not reserve_symbols:
            # a recycled handle.  east_hip_reset gives it the state of a new one but for the build hints (alphabet size,
            # "the window sort took it"): its first build speculates on the previous owner's text as a second build on one
            # handle would.  Results are the same; the plan may differ -- without the planning sample a small repetitive
            # input is not recognised as such (tests/test_gpu_score_exhaustive.py: _Knobs).
            self._h = pooled.pop()
        else:
            _check(self._lib.east_hip_create(self.device, int(reserve_symbols), ctypes.byref(self._h)))
        self.n_docs = 0
        self.doc_offsets = None
        self._host_symbols = None

    @classmethod
    def borrowed(cls, handle, device):
        """A view of a handle somebody else owns (a shard of a HipGroup): close() leaves it alone."""
        self = cls.__new__(cls)
        self._lib = load()
        self._h = ctypes.c_void_p(handle)
        self._borrowed = True
        self.device = int(device)
        self.n_docs = 0
        self.doc_offsets = None
        self._host_symbols = None
        return self

    def close(self):
        """Release the handle.  Handles of small indexes go back to a per-device pool instead of being
        destroyed: stream / event / memory set-up costs more than building a small collection."""
        h = getattr(self, "_h", None)
        if not h:
            return
        self._h = None
        if getattr(self, "_borrowed", False):
            return
        try:
            pool = _handle_pool.setdefault(self.device, [])
            buf = np.zeros(8, dtype=np.int64)
            keep = (len(pool) < POOL_HANDLES and self._lib.east_hip_build_info(h, _ptr(buf, _c_i64p), buf.size) > 6
                    and buf[6] <= POOL_MAX_ARENA_BYTES and self._lib.east_hip_reset(h) == 0)
        except Exception:                        # interpreter shutdown: module globals may be gone
            keep = False
        if keep:
            pool.append(h)
        else:
            self._lib.east_hip_destroy(h)

    __del__ = close

    # -- build ---------------------------------------------------------------
    def build(self, symbols, doc_offsets, n_strings):
        """symbols: the reference encoding (terminator i of a document = 0x0A00+i, text below), or -- told
        by the tag bit of the last symbol -- the tagged one (asts/utils.py: strings_to_symbols)."""
        symbols = np.ascontiguousarray(symbols, dtype=np.uint32)
        doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.int64)
        n_strings = np.ascontiguousarray(n_strings, dtype=np.int32)
        _check(self._lib.east_hip_set_symbol_encoding(self._h, 1 if symbols.size and int(symbols[-1]) >> 31 else 0))
        _check(self._lib.east_hip_build(self._h, _ptr(symbols, _c_u32p), symbols.size, _ptr(doc_offsets, _c_i64p),
                                        _ptr(n_strings, _c_i32p), n_strings.size))
        self.n_docs = int(n_strings.size)
        self.doc_offsets = doc_offsets.copy()
        self._host_symbols = symbols

    def build_device(self, d_symbols_ptr, n_total, doc_offsets, n_strings, tagged=False):
        """d_symbols_ptr: integer address of a uint32 device buffer (e.g. tensor.data_ptr())."""
        doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.int64)
        n_strings = np.ascontiguousarray(n_strings, dtype=np.int32)
        _check(self._lib.east_hip_set_symbol_encoding(self._h, 1 if tagged else 0))
        _check(self._lib.east_hip_build_device(self._h, ctypes.c_void_p(int(d_symbols_ptr)), int(n_total),
                                               _ptr(doc_offsets, _c_i64p), _ptr(n_strings, _c_i32p), n_strings.size))
        self.n_docs = int(n_strings.size)
        self.doc_offsets = doc_offsets.copy()
        self._host_symbols = None

    def build_texts(self, texts):
        """Text preparation + build on the device.  texts: list of bytes (UTF-8, decoded with
        errors='replace' semantics) or str."""
        raw = _raw_texts(texts)
        tables = _table_args()
        if _join_free(raw):
            # a few large texts: uploaded one by one straight out of their bytes objects (joining 64 MiB costs
            # more host time than the device needs for the whole build)
            ptrs, lengths = _separate(raw)
            _check(self._lib.east_hip_build_texts_v(self._h, ptrs, _ptr(lengths, _c_i64p), len(raw), *tables))
        else:
            blob, offsets = _joined(raw)
            _check(self._lib.east_hip_build_texts(self._h, blob, len(blob), _ptr(offsets, _c_i64p), len(raw), *tables))
        self.n_docs = len(raw)
        self._host_symbols = None
        doc_offsets = np.zeros(self.n_docs + 1, dtype=np.int64)
        n_total = ctypes.c_int64(0)
        _check(self._lib.east_hip_get_prepared(self._h, ctypes.byref(n_total), _ptr(doc_offsets, _c_i64p), None, None))
        self.doc_offsets = doc_offsets

    def prepared(self):
        """(symbols uint32, doc_offsets int64, n_strings int32) of the last build_texts.  The symbols are in
        the reference encoding (terminator i = 0x0A00+i) unless kept tokens hold characters at or above
        U+0A00: then in the tagged one (asts/utils.py: is_tagged / reference_code_points)."""
        n_total = ctypes.c_int64(0)
        _check(self._lib.east_hip_get_prepared(self._h, ctypes.byref(n_total), None, None, None))
        doc_offsets = np.zeros(self.n_docs + 1, dtype=np.int64)
        n_strings = np.zeros(self.n_docs, dtype=np.int32)
        symbols = np.zeros(n_total.value, dtype=np.uint32)
        _check(self._lib.east_hip_get_prepared(self._h, ctypes.byref(n_total), _ptr(doc_offsets, _c_i64p),
                                               _ptr(n_strings, _c_i32p), _ptr(symbols, _c_u32p)))
        return symbols, doc_offsets, n_strings

    def symbols(self):
        """The symbols of the index as the host last saw them: kept by build(), fetched from the device
        after build_texts()."""
        if self._host_symbols is None:
            self._host_symbols = self.prepared()[0]
        return self._host_symbols

    @property
    def last_prep_ms(self):
        return float(self._lib.east_hip_last_prep_ms(self._h))

    def tables(self, doc=0, names=("suftab", "lcptab", "anntab", "childtab_up", "childtab_down",
                                   "childtab_next_l_index")):
        order = ("suftab", "lcptab", "anntab", "childtab_up", "childtab_down", "childtab_next_l_index")
        if self.doc_offsets is None or not 0 <= doc < self.n_docs:
            raise exceptions.HipBackendError(reason="no index has been built on this handle, or no such document")
        nd = int(self.doc_offsets[doc + 1] - self.doc_offsets[doc])
        bufs = {k: np.empty(nd, dtype=np.int32) for k in names}
        args = [_ptr(bufs[k], _c_i32p) if k in bufs else None for k in order]
        _check(self._lib.east_hip_get_tables(self._h, int(doc), *args))
        return {k: v.astype(np.int64) for k, v in bufs.items()}    # the reference's np.int dtype

    # -- score ---------------------------------------------------------------
    def score_table(self, q_symbols, q_offsets, normalized=True, want_suffix=False):
        q_symbols = np.ascontiguousarray(q_symbols, dtype=np.uint32)
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.int64)
        K = q_offsets.size - 1
        out = np.empty((K, self.n_docs), dtype=np.float64)
        suf = np.empty((self.n_docs, int(q_offsets[-1])), dtype=np.float64) if want_suffix else None
        _check(self._lib.east_hip_score_table(self._h, _ptr(q_symbols, _c_u32p), _ptr(q_offsets, _c_i64p), K,
                                              int(bool(normalized)), _ptr(out, _c_dblp),
                                              _ptr(suf, _c_dblp) if want_suffix else None))
        return (out, suf) if want_suffix else out

    def score_table_grouped(self, q_symbols, q_offsets, group_offsets, normalized=True):
        """Scores of groups of queries: out[g, d] = max over the queries of group g (synonym variants)."""
        q_symbols = np.ascontiguousarray(q_symbols, dtype=np.uint32)
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.int64)
        group_offsets = np.ascontiguousarray(group_offsets, dtype=np.int64)
        G = group_offsets.size - 1
        out = np.empty((G, self.n_docs), dtype=np.float64)
        _check(self._lib.east_hip_score_table_grouped(self._h, _ptr(q_symbols, _c_u32p), _ptr(q_offsets, _c_i64p),
                                                      q_offsets.size - 1, _ptr(group_offsets, _c_i64p), G,
                                                      int(bool(normalized)), _ptr(out, _c_dblp)))
        return out

    def lcp_interval_lefts(self, doc=0):
        """left[k] = left boundary of the lcp-interval whose first l-index is rank k, -1 for other ranks."""
        if self.doc_offsets is None or not 0 <= doc < self.n_docs:
            raise exceptions.HipBackendError(reason="no index has been built on this handle, or no such document")
        left = np.empty(int(self.doc_offsets[doc + 1] - self.doc_offsets[doc]), dtype=np.int32)
        _check(self._lib.east_hip_get_lcp_intervals(self._h, int(doc), _ptr(left, _c_i32p)))
        return left.astype(np.int64)

    def set_keyphrases(self, q_symbols, q_offsets):
        q_symbols = np.ascontiguousarray(q_symbols, dtype=np.uint32)
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.int64)
        _check(self._lib.east_hip_set_keyphrases(self._h, _ptr(q_symbols, _c_u32p), _ptr(q_offsets, _c_i64p),
                                                 q_offsets.size - 1))

    def score_resident(self, normalized=True, d_out_ptr=None):
        _check(self._lib.east_hip_score_resident(self._h, int(bool(normalized)),
                                                 ctypes.c_void_p(int(d_out_ptr)) if d_out_ptr else None))

    def score_probes(self, normalized=True):
        """Table reads + binary-search probes of one pass of the score walk over the resident keyphrases."""
        c = ctypes.c_int64(0)
        _check(self._lib.east_hip_score_probes(self._h, int(bool(normalized)), ctypes.byref(c)))
        return int(c.value)

    def synchronize(self):
        _check(self._lib.east_hip_synchronize(self._h))

    @property
    def stream(self):
        return self._lib.east_hip_stream(self._h)

    def info(self):
        buf = np.zeros(len(BUILD_INFO_FIELDS), dtype=np.int64)
        self._lib.east_hip_build_info(self._h, _ptr(buf, _c_i64p), buf.size)
        return dict(zip(BUILD_INFO_FIELDS, (int(x) for x in buf)))

    def profile_enable(self, on=True):
        _check(self._lib.east_hip_profile_enable(self._h, int(bool(on))))

    def profile_only(self, kernel=None):
        """Bracket only the launches of `kernel` (None: every kernel) while profiling is enabled."""
        _check(self._lib.east_hip_profile_only(self._h, kernel.encode("ascii") if kernel else None))

    def profile_report(self):
        """{kernel name: (launches, total_ms)} accumulated since profile_enable()."""
        buf = ctypes.create_string_buffer(1 << 16)
        self._lib.east_hip_profile_report(self._h, buf, len(buf))
        out = {}
        for line in buf.value.decode().splitlines():
            name, count, ms = line.split("\t")
            out[name.strip("()")] = (int(count), float(ms))
        return out

    @property
    def last_build_ms(self):
        return float(self._lib.east_hip_last_build_ms(self._h))

    @property
    def last_score_ms(self):
        return float(self._lib.east_hip_last_score_ms(self._h))

    # -- text-to-text relatedness ----------------------------------------------
    def related_build(self, normalized=True, orientation=RELATED_SYMMETRIC):
        """The D x D relatedness matrix of the index's own texts (include/east_hip.h, "Text-to-text relatedness"): every
        string of text A scored against the tree of text B, averaged per A; it stays on the device.  The call replaces the
        resident keyphrases.  -> (D, scored strings, score launches)"""
        out = np.zeros(3, dtype=np.int64)
        _check(self._lib.east_hip_related_build(self._h, int(bool(normalized)), int(orientation), _ptr(out, _c_i64p)))
        self._rel_M = int(out[0])
        return int(out[0]), int(out[1]), int(out[2])

    def related_matrix(self):
        """The last relatedness matrix of this handle -> (matrix[D, D] with NaN on the diagonal, self[D] = F[A][A],
        scored[D] = the scored strings of every text, int32)."""
        return _matrix_fetch(self._lib.east_hip_related_fetch, self._h, self._rel_M)

    def rank_related(self, n, threshold=-np.inf):
        """A ranking of the last relatedness matrix by row (other n, other threshold: no new matrix) -> TopArrays."""
        return _top_build(self._lib, self._h, GRAPH_SOURCE_RELATED, None, TOP_BY_KEYPHRASE, n, threshold)

    def related(self, normalized=True, orientation=RELATED_SYMMETRIC, n=10, threshold=-np.inf):
        """related_build, then the n most related other texts of every text (the NaN on the diagonal is never eligible)
        -> TopArrays.  It is the handle's one ranking: it replaces top()'s and similar()'s."""
        self.related_build(normalized, orientation)
        return self.rank_related(n, threshold)

    def last_related_ms(self):
        return float(self._lib.east_hip_last_related_ms(self._h))

    # -- tables from elsewhere: each consumer keeps an uploaded copy of its own ------
    def graph_from_table(self, table, rows, relevance_threshold, support_threshold, referral_confidence):
        """The same from a K x D host array, which is uploaded first (tables from elsewhere, tests)."""
        return _graph_build(self._lib, self._h, None, table, rows, relevance_threshold, support_threshold,
                            referral_confidence)

    def graph_from_uploaded(self, rows, relevance_threshold, support_threshold, referral_confidence):
        """Another graph of the table graph_from_table left on the device: no upload."""
        return _graph_build(self._lib, self._h, GRAPH_SOURCE_UPLOADED, None, rows, relevance_threshold, support_threshold,
                            referral_confidence)

    def top_from_table(self, table, axis, n, threshold=-np.inf):
        """The same from a K x D host array, which is uploaded first (tables from elsewhere, tests)."""
        return _top_build(self._lib, self._h, None, table, axis, n, threshold)

    def top_from_uploaded(self, axis, n, threshold=-np.inf):
        """Another ranking of the table top_from_table left on the device: no upload."""
        return _top_build(self._lib, self._h, GRAPH_SOURCE_UPLOADED, None, axis, n, threshold)

    def similarity_from_table(self, table, axis):
        """The same from a K x D host array, which is uploaded first (tables from elsewhere, tests)."""
        return self._similarity(None, table, axis)

    def similarity_from_uploaded(self, axis):
        """Another matrix (the other axis) of the table similarity_from_table left on the device: no upload."""
        return self._similarity(GRAPH_SOURCE_UPLOADED, None, axis)


class HipCosineIndex(_ResidentTableConsumers):
    """The cosine measure's term index (include/east_hip.h, "The cosine relevance measure"): the postings (term, document,
    count) of a whole collection, built on the device from raw texts.  It lives in the handle of a HipIndex: its own one
    (device choice and handle pool as HipIndex) unless `index` is given -- then it shares that handle, whose EASA index it
    leaves alone, and closing is the owner's business."""

    _table_source = GRAPH_SOURCE_COSINE          # graph(), top(), similarity(): of the table the last score_table left

    def __init__(self, device=None, index=None):
        self._owner = index is None
        self.index = HipIndex(device) if index is None else index
        self._lib = self.index._lib
        self.device = self.index.device
        self.n_docs = 0
        self.n_terms = 0

    @property
    def _h(self):
        return self.index._h

    @property
    def _sim_holder(self):
        return self.index

    def close(self):
        if self._owner:
            self.index.close()

    def build_texts(self, texts, stopwords=()):
        """texts: bytes (UTF-8, decoded with errors='replace') or str; stopwords: upper-cased words."""
        raw = _raw_texts(texts)
        sw_cps, sw_off = pack_words(list(stopwords))
        args = _table_args() + (_ptr(sw_cps, _c_u32p), _ptr(sw_off, _c_i64p), sw_off.size - 1)
        if _join_free(raw):
            ptrs, lengths = _separate(raw)
            _check(self._lib.east_hip_cosine_build_texts_v(self._h, ptrs, _ptr(lengths, _c_i64p), len(raw), *args))
        else:
            blob, offsets = _joined(raw)
            _check(self._lib.east_hip_cosine_build_texts(self._h, blob, len(blob), _ptr(offsets, _c_i64p), len(raw), *args))
        self.n_docs = len(raw)
        self.n_terms = self.info()["terms"]

    def info(self):
        buf = np.zeros(len(COSINE_INFO_FIELDS), dtype=np.int64)
        _check(self._lib.east_hip_cosine_info(self._h, _ptr(buf, _c_i64p), buf.size))
        return dict(zip(COSINE_INFO_FIELDS, (int(x) for x in buf)))

    def terms(self, tfidf=None, n=None, min_texts=1, groups=None, n_groups=None):
        """Without arguments: the terms in id order (first occurrence in the collection).
        terms(tfidf, n, min_texts, groups=None): the characteristic terms of every text (groups None) or of every group of
        texts (groups[d] = the group of text d in 0 .. n_groups - 1, n_groups None: max(groups) + 1; include/east_hip.h,
        "Characteristic terms") -> TermArrays."""
        if n is not None:
            return self._characteristic_terms(tfidf, n, min_texts, groups, n_groups)
        n = ctypes.c_int64(0)
        _check(self._lib.east_hip_cosine_get_terms(self._h, None, None, ctypes.byref(n)))
        offsets = np.zeros(self.n_terms + 1, dtype=np.int64)
        cps = np.zeros(max(n.value, 1), dtype=np.uint32)
        _check(self._lib.east_hip_cosine_get_terms(self._h, _ptr(offsets, _c_i64p), _ptr(cps, _c_u32p), ctypes.byref(n)))
        text = cps[:n.value].astype("<u4").tobytes().decode("utf-32-le", errors="surrogatepass")
        return [text[offsets[t]:offsets[t + 1]] for t in range(self.n_terms)]

    def set_classes(self, term_class, n_classes):
        """The vector space of classes of terms (stems): term_class[t], classes numbered by their smallest term id;
        n_classes = 0 goes back to the terms."""
        tc = np.ascontiguousarray(term_class, dtype=np.int32)
        _check(self._lib.east_hip_cosine_set_classes(self._h, _ptr(tc, _c_i32p) if n_classes else None, int(n_classes)))

    def lookup(self, words):
        """[prepared word] -> int32 term ids, -1 for a word that is not a term."""
        out = np.full(len(words), -1, dtype=np.int32)
        if words:
            cps, offsets = pack_words(words)
            _check(self._lib.east_hip_cosine_lookup(self._h, _ptr(cps, _c_u32p), _ptr(offsets, _c_i64p), len(words),
                                                    _ptr(out, _c_i32p)))
        return out

    def score_table(self, q_ids, q_offsets, tfidf=True, fetch=True):
        """K x D cosine scores: q_ids[q_offsets[k]:q_offsets[k + 1]] = the kept tokens of query k as ids of the vector
        space, -1 outside it.  fetch=False: the table stays on the device (for graph()), nothing is returned."""
        q_ids = np.ascontiguousarray(q_ids, dtype=np.int32)
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.int64)
        K = q_offsets.size - 1
        out = np.empty((K, self.n_docs), dtype=np.float64) if fetch else None
        _check(self._lib.east_hip_cosine_score_table(self._h, _ptr(q_ids, _c_i32p), _ptr(q_offsets, _c_i64p), q_ids.size, K,
                                                     1 if tfidf else 0, _ptr(out, _c_dblp) if fetch else None))
        return out

    # -- BM25: a second score call of the same index ------------------------------
    def bm25_table(self, q_ids, q_offsets, k1=1.2, b=0.75, fetch=True):
        """K x D BM25 scores (include/east_hip.h, "BM25") of the queries score_table takes; the table replaces the last
        score call's on the device.  fetch=False: it stays there, nothing is returned."""
        q_ids = np.ascontiguousarray(q_ids, dtype=np.int32)
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.int64)
        K = q_offsets.size - 1
        out = np.empty((K, self.n_docs), dtype=np.float64) if fetch else None
        _check(self._lib.east_hip_bm25_score_table(self._h, _ptr(q_ids, _c_i32p), _ptr(q_offsets, _c_i64p), q_ids.size, K,
                                                   float(k1), float(b), _ptr(out, _c_dblp) if fetch else None))
        return out

    def bm25_info(self):
        """{BM25_INFO_FIELDS: value}: N and weights_computed as int, the rest float."""
        buf = np.zeros(len(BM25_INFO_FIELDS), dtype=np.float64)
        _check(self._lib.east_hip_bm25_info(self._h, _ptr(buf, _c_dblp), buf.size))
        info = dict(zip(BM25_INFO_FIELDS, (float(x) for x in buf)))
        info["N"], info["weights_computed"] = int(info["N"]), int(info["weights_computed"])
        return info

    # -- text-to-text cosine similarity ------------------------------------------
    def texts_build(self, tfidf=True):
        """The D x D cosine matrix of the index's own texts in the vector space the score call uses (include/east_hip.h,
        "Text-to-text cosine similarity"); it stays on the device.  -> {COSINE_TEXTS_INFO_FIELDS: value}"""
        out = np.zeros(len(COSINE_TEXTS_INFO_FIELDS), dtype=np.int64)
        _check(self._lib.east_hip_text_similarity_build(self._h, 1 if tfidf else 0, _ptr(out, _c_i64p)))
        self._texts_M = int(out[0])
        return dict(zip(COSINE_TEXTS_INFO_FIELDS, (int(x) for x in out)))

    def texts_matrix(self):
        """The last text-to-text cosine matrix of this handle -> (matrix[D, D] with NaN on the diagonal, self[D] = the
        diagonal before the NaN, postings[D] = the postings of every text, int32)."""
        return _matrix_fetch(self._lib.east_hip_text_similarity_fetch, self._h, self._texts_M)

    def rank_texts(self, n, threshold=-np.inf):
        """A ranking of the last text-to-text cosine matrix by row (other n, other threshold: no new matrix) -> TopArrays."""
        return _top_build(self._lib, self._h, GRAPH_SOURCE_COSINE_TEXTS, None, TOP_BY_KEYPHRASE, n, threshold)

    def texts_similar(self, tfidf=True, n=10, threshold=-np.inf):
        """texts_build, then the n most similar other texts of every text (the NaN on the diagonal is never eligible)
        -> TopArrays.  It is the handle's one ranking: it replaces top()'s and similar()'s."""
        self.texts_build(tfidf)
        return self.rank_texts(n, threshold)

    def last_texts_ms(self):
        return float(self._lib.east_hip_last_text_similarity_ms(self._h))

    # -- shingle overlap -----------------------------------------------------------
    def overlap_build(self, words=4, orientation=OVERLAP_SYMMETRIC):
        """The D x D matrix of the shared w-word shingles of the index's own texts: the resemblance (symmetric) or the
        containment of the row's text in the column's (directed; include/east_hip.h, "Shingle overlap"); it stays on the
        device.  -> {OVERLAP_INFO_FIELDS: value}"""
        out = np.zeros(len(OVERLAP_INFO_FIELDS), dtype=np.int64)
        _check(self._lib.east_hip_overlap_build(self._h, int(words), int(orientation), _ptr(out, _c_i64p)))
        self._overlap_M = int(out[0])
        return dict(zip(OVERLAP_INFO_FIELDS, (int(x) for x in out)))

    def overlap_matrix(self):
        """The last overlap matrix of this handle -> (matrix[D, D] with NaN on the diagonal, self[D] = the diagonal before
        the NaN, shingles[D] = the distinct shingles of every text, int32)."""
        return _matrix_fetch(self._lib.east_hip_overlap_fetch, self._h, self._overlap_M)

    def rank_overlap(self, n, threshold=-np.inf):
        """A ranking of the last overlap matrix by row (other n, other threshold: no new matrix) -> TopArrays."""
        return _top_build(self._lib, self._h, GRAPH_SOURCE_OVERLAP, None, TOP_BY_KEYPHRASE, n, threshold)

    def texts_overlap(self, words=4, orientation=OVERLAP_SYMMETRIC, n=10, threshold=-np.inf):
        """overlap_build, then the n other texts every text shares most with -> TopArrays (the handle's one ranking)."""
        self.overlap_build(words, orientation)
        return self.rank_overlap(n, threshold)

    def last_overlap_ms(self):
        return float(self._lib.east_hip_last_overlap_ms(self._h))

    # -- shared passages -----------------------------------------------------------
    def passages(self, pairs_a, pairs_b, words=4, min_words=None, per_pair=5):
        """The passages of text pairs_a[i] whose every `words` consecutive words occur in text pairs_b[i] (include/east_hip.h,
        "Shared passages"): per pair the passages of min_words words or more (None: `words`), longest first, per_pair of
        them at most (0: all) -> PassageArrays."""
        return _passages(self._lib, self._h, pairs_a, pairs_b, words, words if min_words is None else min_words, per_pair)

    def passages_phases_ms(self):
        """(names and postings, the match kernel, runs + order + cut) of the last passages build, device ms."""
        ms = np.zeros(3, dtype=np.float64)
        _check(self._lib.east_hip_passages_phases(self._h, _ptr(ms, _c_dblp)))
        return tuple(float(x) for x in ms)

    def last_passages_ms(self):
        return float(self._lib.east_hip_last_passages_ms(self._h))

    # -- characteristic terms ------------------------------------------------------
    def _characteristic_terms(self, tfidf, n, min_texts, groups, n_groups=None):
        group = None if groups is None else np.ascontiguousarray(groups, dtype=np.int32)
        if n_groups is None:
            n_groups = self.n_docs if group is None else (int(group.max()) + 1 if group.size else 0)
        out = np.zeros(len(TERMS_INFO_FIELDS), dtype=np.int64)
        _check(self._lib.east_hip_terms_build(self._h, 1 if tfidf else 0, None if group is None else _ptr(group, _c_i32p),
                                              int(n_groups), int(n), int(min_texts), _ptr(out, _c_i64p)))
        G, n = int(out[1]), int(n)
        self._terms_info = dict(zip(TERMS_INFO_FIELDS, (int(x) for x in out)))
        found = TermArrays(np.empty(G, np.int32), np.empty(G, np.int32), np.empty((G, n), np.int32), np.empty((G, n), np.float64),
                           np.empty((G, n), np.int32), np.empty((G, n), np.int32), self._terms_info)
        _check(self._lib.east_hip_terms_fetch(self._h, _ptr(found.members, _c_i32p), _ptr(found.count, _c_i32p),
                                              _ptr(found.unit, _c_i32p), _ptr(found.value, _c_dblp), _ptr(found.texts, _c_i32p),
                                              _ptr(found.df, _c_i32p)))
        return found

    def terms_vectors(self):
        """Every entry of the last terms() build before min_texts and the cut, in (group, unit) order
        -> (offsets[G + 1] int64, unit int32, value float64, texts int32)."""
        G, E = self._terms_info["groups"], self._terms_info["entries"]
        offsets, unit = np.zeros(G + 1, np.int64), np.empty(E, np.int32)
        value, texts = np.empty(E, np.float64), np.empty(E, np.int32)
        _check(self._lib.east_hip_terms_fetch_vectors(self._h, _ptr(offsets, _c_i64p), _ptr(unit, _c_i32p), _ptr(value, _c_dblp),
                                                      _ptr(texts, _c_i32p)))
        return offsets, unit, value, texts

    def last_terms_ms(self):
        return float(self._lib.east_hip_last_terms_ms(self._h))


SYNONYMS_INFO_FIELDS = ("raw_triples", "distinct_triples", "words", "relations", "features", "longest_row")


class HipSynonyms(object):
    """The feature rows of a SynonymExtractor on the device (include/east_hip.h, "Synonym extraction"): built from interned
    dependency triples, queried for rows, similarities and all pairs of candidates above a threshold.  It lives in the
    handle of a HipIndex, as HipCosineIndex does: its own one unless `index` is given."""

    def __init__(self, device=None, index=None):
        self._owner = index is None
        self.index = HipIndex(device) if index is None else index
        self._lib = self.index._lib
        self.device = self.index.device
        self.n_words = 0

    @property
    def _h(self):
        return self.index._h

    def close(self):
        if self._owner:
            self.index.close()

    def build(self, w1, relation, w2, inverse_relation, n_words):
        """The raw triples as int32 id arrays; inverse_relation[r] = the id of r's inverse (synonyms.py:81)."""
        w1, relation, w2, inverse_relation = (np.ascontiguousarray(x, dtype=np.int32) for x in (w1, relation, w2, inverse_relation))
        if not (w1.size == relation.size == w2.size):
            raise exceptions.HipBackendError(reason="the three id arrays of the triples differ in length")
        _check(self._lib.east_hip_synonyms_build(self._h, _ptr(w1, _c_i32p), _ptr(relation, _c_i32p), _ptr(w2, _c_i32p), w1.size,
                                                 _ptr(inverse_relation, _c_i32p), int(n_words), inverse_relation.size))
        self.n_words = int(n_words)

    def info(self):
        buf = np.zeros(len(SYNONYMS_INFO_FIELDS), dtype=np.int64)
        _check(self._lib.east_hip_synonyms_info(self._h, _ptr(buf, _c_i64p), buf.size))
        return dict(zip(SYNONYMS_INFO_FIELDS, (int(x) for x in buf)))

    def rows(self):
        """(offsets int64[n_words + 1], relation int32[F], word int32[F], I float64[F], row_sum float64[n_words])."""
        info = self.info()
        F, W = info["features"], info["words"]
        offsets = np.zeros(W + 1, dtype=np.int64)
        relation, word = np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.int32)
        value, row_sum = np.zeros(F, dtype=np.float64), np.zeros(W, dtype=np.float64)
        _check(self._lib.east_hip_synonyms_get_rows(self._h, _ptr(offsets, _c_i64p), _ptr(relation, _c_i32p), _ptr(word, _c_i32p),
                                                    _ptr(value, _c_dblp), _ptr(row_sum, _c_dblp)))
        return offsets, relation, word, value, row_sum

    def similarity(self, a, b):
        """similarity(a[i], b[i]) of word ids -> float64."""
        a, b = np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(b, dtype=np.int32)
        if a.size != b.size:
            raise exceptions.HipBackendError(reason="the two id arrays of the pairs differ in length")
        out = np.zeros(a.size, dtype=np.float64)
        _check(self._lib.east_hip_synonyms_similarity(self._h, _ptr(a, _c_i32p), _ptr(b, _c_i32p), a.size, _ptr(out, _c_dblp)))
        return out

    def pairs(self, candidates, threshold, fetch=True):
        """Every pair (i < j in list order) of the candidate word ids with similarity > threshold ->
        (a int32, b int32, similarity float64), ordered by i, then j; fetch=False: only their number."""
        candidates = np.ascontiguousarray(candidates, dtype=np.int32)
        n = ctypes.c_int64(0)
        _check(self._lib.east_hip_synonyms_pairs(self._h, _ptr(candidates, _c_i32p), candidates.size, float(threshold),
                                                 ctypes.byref(n)))
        if not fetch:
            return int(n.value)
        a, b = np.zeros(n.value, dtype=np.int32), np.zeros(n.value, dtype=np.int32)
        sim = np.zeros(n.value, dtype=np.float64)
        _check(self._lib.east_hip_synonyms_fetch(self._h, _ptr(a, _c_i32p), _ptr(b, _c_i32p), _ptr(sim, _c_dblp)))
        return a, b, sim

    @property
    def last_ms(self):
        return float(self._lib.east_hip_last_synonyms_ms(self._h))


class HipGroup(object):
    """One collection over several devices in this process: a shard of documents -- one HipIndex -- per device, driven
    by the library's own host threads, the K x D_local score blocks assembled by one all-gather (RCCL between distinct
    devices; include/east_hip.h, "Several devices in one process").  `devices`: a count (devices 0 .. N-1) or a list of
    ordinals; an ordinal may appear several times (logical shards on one device)."""

    def __init__(self, devices):
        self._lib = load()
        self.devices = list(range(devices)) if isinstance(devices, int) else [int(d) for d in devices]
        if not self.devices:
            raise exceptions.HipBackendError(reason="a device group needs at least one device")
        self._g = ctypes.c_void_p()
        dev = np.array(self.devices, dtype=np.int32)
        _check(self._lib.east_hip_group_create(_ptr(dev, _c_i32p), dev.size, ctypes.byref(self._g)))
        self.n_docs = 0
        self.first_doc = None
        self.shards = []

    def close(self):
        g = getattr(self, "_g", None)
        if g:
            self._g = None
            for shard in self.shards:
                shard.close()
            self._lib.east_hip_group_destroy(g)

    __del__ = close

    def _after_build(self, n_docs):
        self.n_docs = int(n_docs)
        first = np.zeros(len(self.devices) + 1, dtype=np.int32)
        self._lib.east_hip_group_shards(self._g, _ptr(first, _c_i32p))
        self.first_doc = first
        self.shards = []
        for s, device in enumerate(self.devices):
            view = HipIndex.borrowed(self._lib.east_hip_group_handle(self._g, s), device)
            view.n_docs = int(first[s + 1] - first[s])
            if view.n_docs:
                offsets = np.zeros(view.n_docs + 1, dtype=np.int64)
                n_total = ctypes.c_int64(0)
                if self._from_texts:
                    _check(self._lib.east_hip_get_prepared(view._h, ctypes.byref(n_total), _ptr(offsets, _c_i64p), None, None))
                else:
                    b, e = int(first[s]), int(first[s + 1])
                    offsets = (self._doc_offsets[b:e + 1] - self._doc_offsets[b]).astype(np.int64)
                    view._host_symbols = self._symbols[int(self._doc_offsets[b]):int(self._doc_offsets[e])]
                view.doc_offsets = offsets
            self.shards.append(view)

    def build(self, symbols, doc_offsets, n_strings):
        symbols = np.ascontiguousarray(symbols, dtype=np.uint32)
        doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.int64)
        n_strings = np.ascontiguousarray(n_strings, dtype=np.int32)
        tagged = 1 if symbols.size and int(symbols[-1]) >> 31 else 0
        _check(self._lib.east_hip_group_build(self._g, _ptr(symbols, _c_u32p), symbols.size, _ptr(doc_offsets, _c_i64p),
                                              _ptr(n_strings, _c_i32p), n_strings.size, tagged))
        self._from_texts, self._symbols, self._doc_offsets = False, symbols, doc_offsets
        self._after_build(n_strings.size)

    def build_texts(self, texts):
        raw = _raw_texts(texts)
        ptrs, lengths = _separate(raw)
        _check(self._lib.east_hip_group_build_texts_v(self._g, ptrs, _ptr(lengths, _c_i64p), len(raw), *_table_args()))
        self._from_texts = True
        self._after_build(len(raw))

    def locate(self, doc):
        """(shard view, document number inside the shard) of document `doc` of the collection."""
        s = int(np.searchsorted(self.first_doc, doc, side="right")) - 1
        return self.shards[s], int(doc - self.first_doc[s])

    def score_table(self, q_symbols, q_offsets, normalized=True):
        q_symbols = np.ascontiguousarray(q_symbols, dtype=np.uint32)
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.int64)
        K = q_offsets.size - 1
        out = np.empty((K, self.n_docs), dtype=np.float64)
        _check(self._lib.east_hip_score_table_multi(self._g, _ptr(q_symbols, _c_u32p), _ptr(q_offsets, _c_i64p), K,
                                                    int(bool(normalized)), _ptr(out, _c_dblp)))
        return out

    def info(self):
        buf = np.zeros(5, dtype=np.float64)
        self._lib.east_hip_group_info(self._g, _ptr(buf, _c_dblp), buf.size)
        return {"build_ms": float(buf[0]), "score_ms": float(buf[1]), "gather_ms": float(buf[2]),
                "gather": {1: "rccl", 2: "copies"}.get(int(buf[3]), None), "shards": int(buf[4])}


def shard_documents(sizes, n_shards):
    """The library's sharding rule (host only): first_doc[n_shards + 1]."""
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    first = np.zeros(n_shards + 1, dtype=np.int32)
    _check(load().east_hip_debug_shard_documents(_ptr(sizes, _c_i64p), sizes.size, n_shards, _ptr(first, _c_i32p)))
    return first


def format_table(scores, kp_order, text_order, kp_names, text_names, kind):
    """The keyphrase table as text through the library's host-side formatter (east_hip_format_table_xml / _csv): scores
    K x D float64, the output order of rows / columns as index arrays, names as str (CSV: already quoted)."""
    lib = load()
    scores = np.ascontiguousarray(scores, dtype=np.float64)
    K, D = scores.shape
    kp_order = np.ascontiguousarray(kp_order, dtype=np.int32)
    text_order = np.ascontiguousarray(text_order, dtype=np.int32)
    kp_b = [s.encode("utf-8", "surrogatepass") for s in kp_names]
    text_b = [s.encode("utf-8", "surrogatepass") for s in text_names]
    if any(b"\0" in b for b in kp_b) or any(b"\0" in b for b in text_b):
        raise ValueError("NUL in a name")
    fn = lib.east_hip_format_table_xml if kind == "xml" else lib.east_hip_format_table_csv
    cap = 64 + sum(len(b) + 64 for b in kp_b) + (sum(len(b) + 64 for b in text_b) + 8) * max(K, 1) + 40 * K * D
    buf = ctypes.create_string_buffer(cap)
    n = fn(_ptr(scores, _c_dblp), K, D, _ptr(kp_order, _c_i32p), _ptr(text_order, _c_i32p),
           (ctypes.c_char_p * max(K, 1))(*kp_b), (ctypes.c_char_p * max(D, 1))(*text_b), buf, cap)
    if n < 0:
        raise exceptions.HipBackendError(reason="table formatter: %d" % n)
    return buf.raw[:n].decode("utf-8", "surrogatepass")


def pack_words(words):
    """[str] -> (code points uint32, offsets int64)."""
    cps = np.frombuffer("".join(words).encode("utf-32-le", errors="surrogatepass"), dtype="<u4").astype(np.uint32)
    offsets = np.zeros(len(words) + 1, dtype=np.int64)
    np.cumsum([len(w) for w in words], out=offsets[1:])
    return cps, offsets


def pack_queries(queries, keep_spaces=False):
    """[unicode query] -> (q_symbols uint32, q_offsets int64); U+0020 is removed as score() does
    (easa.py:36) unless keep_spaces (synonym variants go to _score as they are, easa.py:34)."""
    from east.asts import utils as ast_utils
    parts = [ast_utils.query_to_symbols(q, keep_spaces) for q in queries]
    offsets = np.zeros(len(parts) + 1, dtype=np.int64)
    for i, p in enumerate(parts):
        offsets[i + 1] = offsets[i] + p.size
    symbols = np.concatenate(parts) if parts else np.zeros(0, np.uint32)
    return symbols.astype(np.uint32), offsets
