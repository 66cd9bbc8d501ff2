"""ctypes binding of libcphnsw_mi355x.so — exactly the symbols include/cphnsw_mi355x.h declares."""
import ctypes as C
import importlib.util
import os
import sys

from . import build as _build

OK, INVALID_ARGUMENT, RUNTIME_ERROR, OUT_OF_MEMORY, NOT_IMPLEMENTED = range(5)
IDS_INTERNAL, IDS_INPUT = 0, 1      # cph_set_result_ids
METRIC_L2, METRIC_COSINE = 0, 1     # cph_set_metric
METRIC_IP = 2

# name -> (restype, argtypes); the list is checked against the header by tests/test_abi.py
SYMBOLS = {
    "cph_last_error": (C.c_char_p, []),
    "cph_version": (C.c_int, []),
    "cph_create": (C.c_int, [C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]),
    "cph_destroy": (C.c_int, [C.c_void_p]),
    "cph_load": (C.c_int, [C.c_void_p, C.c_char_p]),
    "cph_save": (C.c_int, [C.c_void_p, C.c_char_p]),
    "cph_save_native": (C.c_int, [C.c_void_p, C.c_char_p]),
    "cph_load_native": (C.c_int, [C.c_void_p, C.c_char_p]),
    "cph_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cph_dim": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cph_is_finalized": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "cph_build": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "cph_finalize": (C.c_int, [C.c_void_p]),
    "cph_knn_bruteforce": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
                                     C.c_void_p, C.c_void_p]),
    "cph_debug_knn": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_int,
                                C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "cph_host_knn": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_int,
                               C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]),
    "cph_debug_heap_ops": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "cph_debug_estimator": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                      C.c_void_p, C.c_uint32, C.c_void_p]),
    "cph_select_hook": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64,
                                  C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_select_layer_hook": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_float, C.c_float,
                                        C.c_float, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_calib_hook": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_encode_edges": (C.c_int, [C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "cph_search_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "cph_search_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "cph_filter_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "cph_filter_destroy": (C.c_int, [C.c_void_p]),
    "cph_search_batch_filtered": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "cph_search_batch_device_filtered": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_search_batch_exact": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "cph_search_batch_exact_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_set_exact_threshold": (C.c_int, [C.c_void_p, C.c_uint64]),
    "cph_search_batch_filters": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                           C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "cph_search_batch_filters_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                                  C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_multi_search_batch_filters": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                                 C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "cph_host_filter_groups": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_uint64,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_host_exact_group_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_uint64, C.c_void_p,
                                            C.c_uint64, C.c_void_p]),
    "cph_multi_search_batch_exact": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                               C.c_void_p, C.c_void_p]),
    "cph_multi_set_exact_threshold": (C.c_int, [C.c_void_p, C.c_uint64]),
    "cph_host_filter_ids": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]),
    "cph_host_exact_plan": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cph_range_search_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64,
                                         C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "cph_range_search_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "cph_range_destroy": (C.c_int, [C.c_void_p]),
    "cph_multi_range_search_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64,
                                               C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "cph_multi_range_search_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_multi_range_destroy": (C.c_int, [C.c_void_p]),
    "cph_host_range_plan": (C.c_int, [C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]),
    "cph_host_range_tiles": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]),
    "cph_host_range_merge_pass": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "cph_group_keys_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]),
    "cph_group_keys_destroy": (C.c_int, [C.c_void_p]),
    "cph_search_grouped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int,
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_search_grouped_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int,
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_multi_search_grouped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int,
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_debug_time_grouped": (C.c_int, [C.c_void_p, C.c_int]),
    "cph_debug_last_group_rows_us": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "cph_group_rows_hook": (C.c_int, [C.c_int] + [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64,
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_host_group_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64,
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_search_diverse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_float, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int,
        C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_search_diverse_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_float, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int,
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_multi_search_diverse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_float, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int,
        C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_debug_time_diverse": (C.c_int, [C.c_void_p, C.c_int]),
    "cph_debug_last_diverse_rows_us": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "cph_diverse_rows_hook": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_host_diverse_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
        C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_search_maxsim": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
        C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_search_maxsim_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
        C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_multi_search_maxsim": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
        C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_debug_time_maxsim": (C.c_int, [C.c_void_p, C.c_int]),
    "cph_debug_last_maxsim_rows_us": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "cph_maxsim_rows_hook": (C.c_int, [C.c_int] + [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
        C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_host_maxsim_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
        C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_search_maxsim_rescored": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
        C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_search_maxsim_rescored_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
        C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_multi_search_maxsim_rescored": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
        C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_prepare_maxsim_rescore": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cph_debug_time_maxsim_rescore": (C.c_int, [C.c_void_p, C.c_int]),
    "cph_debug_last_maxsim_rescore_us": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "cph_maxsim_rescore_hook": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
        C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_host_maxsim_rescore": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
        C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
        C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_host_key_rows": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "cph_search_fused": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
        C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_search_fused_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
        C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_multi_search_fused": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
        C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_debug_time_fused": (C.c_int, [C.c_void_p, C.c_int]),
    "cph_debug_last_fused_us": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "cph_fused_rows_hook": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
        C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_host_fused_rows": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
        C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_filter_create_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "cph_has_row_map": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "cph_get_row_map": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "cph_set_row_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "cph_set_result_ids": (C.c_int, [C.c_void_p, C.c_int]),
    "cph_remove": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]),
    "cph_live_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cph_get_removed": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cph_compact": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cph_host_live_filter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]),
    "cph_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_int64)]),
    "cph_tail_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cph_tail_fold_hook": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                     C.c_uint32, C.c_void_p, C.c_void_p]),
    "cph_host_tail_fold": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                     C.c_void_p, C.c_void_p]),
    "cph_host_tail_capacity": (C.c_int, [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cph_multi_remove": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]),
    "cph_multi_live_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cph_multi_get_removed": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cph_multi_compact": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cph_parts_remove": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cph_parts_live_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cph_parts_get_removed": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cph_parts_compact": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cph_set_labels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]),
    "cph_has_labels": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "cph_get_labels": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "cph_filters_from_labels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "cph_debug_time_label_filters": (C.c_int, [C.c_void_p, C.c_int]),
    "cph_debug_last_label_filters_us": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "cph_filter_export": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "cph_host_label_filters": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "cph_multi_set_labels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]),
    "cph_parts_set_labels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "cph_parts_filters_from_labels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "cph_parts_filter_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cph_filters_combine": (C.c_int, [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "cph_parts_filters_combine": (C.c_int, [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "cph_host_filter_combine": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    "cph_filter_combine_hook": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_uint32, C.c_void_p,
                                          C.c_void_p, C.POINTER(C.c_double)]),
    "cph_set_column": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int]),
    "cph_has_column": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_int)]),
    "cph_get_column": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]),
    "cph_filters_from_column": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "cph_multi_set_column": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int]),
    "cph_parts_set_column": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]),
    "cph_parts_filters_from_column": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "cph_set_tags": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]),
    "cph_has_tags": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_int)]),
    "cph_get_tags": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "cph_filters_from_tags": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "cph_debug_time_tag_filters": (C.c_int, [C.c_void_p, C.c_int]),
    "cph_debug_last_tag_filters_us": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "cph_host_tag_filters": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                       C.c_void_p]),
    "cph_facet_onchip_limit": (C.c_int, []),
    "cph_facet_slab_counters": (C.c_uint64, []),
    "cph_facet_prepare": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32]),
    "cph_facet_values": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.POINTER(C.c_uint64), C.c_void_p]),
    "cph_facet_counts": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "cph_facet_top": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_debug_time_facets": (C.c_int, [C.c_void_p, C.c_int]),
    "cph_debug_last_facets_us": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "cph_debug_facet_slab": (C.c_int, [C.c_void_p, C.c_uint64]),
    "cph_host_facet_values": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]),
    "cph_host_facet_counts": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "cph_host_facet_top": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_facet_hook": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int,
                                 C.c_void_p, C.POINTER(C.c_double)]),
    "cph_multi_set_tags": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]),
    "cph_parts_set_tags": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64]),
    "cph_parts_filters_from_tags": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "cph_synchronize": (C.c_int, [C.c_void_p]),
    "cph_set_batch_sets": (C.c_int, [C.c_void_p, C.c_uint32]),
    "cph_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                             C.POINTER(C.c_uint64)]),
    "cph_get_vectors": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "cph_set_search_params": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64]),
    "cph_last_search_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cph_last_query_expansions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "cph_order_queries": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "cph_multi_create": (C.c_int, [C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "cph_multi_destroy": (C.c_int, [C.c_void_p]),
    "cph_multi_load": (C.c_int, [C.c_void_p, C.c_char_p]),
    "cph_multi_load_native": (C.c_int, [C.c_void_p, C.c_char_p]),
    "cph_multi_save": (C.c_int, [C.c_void_p, C.c_char_p]),
    "cph_multi_save_native": (C.c_int, [C.c_void_p, C.c_char_p]),
    "cph_multi_build": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "cph_multi_finalize": (C.c_int, [C.c_void_p]),
    "cph_multi_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cph_multi_is_finalized": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "cph_multi_search_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "cph_multi_search_batch_filtered": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]),
    "cph_multi_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_uint64)]),
    "cph_multi_has_row_map": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "cph_multi_set_row_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "cph_multi_set_result_ids": (C.c_int, [C.c_void_p, C.c_int]),
    "cph_multi_set_min_shard": (C.c_int, [C.c_void_p, C.c_uint64]),
    "cph_multi_last_search_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cph_multi_last_query_expansions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "cph_multi_num_replicas": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "cph_multi_replica": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "cph_parts_create": (C.c_int, [C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "cph_parts_destroy": (C.c_int, [C.c_void_p]),
    "cph_parts_build": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "cph_parts_finalize": (C.c_int, [C.c_void_p]),
    "cph_parts_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cph_parts_is_finalized": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "cph_parts_save_native": (C.c_int, [C.c_void_p, C.c_char_p]),
    "cph_parts_load_native": (C.c_int, [C.c_void_p, C.c_char_p]),
    "cph_parts_search_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "cph_parts_search_batch_filtered": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                                  C.c_void_p]),
    "cph_parts_search_batch_exact": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                               C.c_void_p]),
    "cph_parts_search_batch_filters": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                                 C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "cph_parts_search_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                                C.c_void_p]),
    "cph_parts_search_batch_device_filtered": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_parts_search_batch_exact_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_parts_search_batch_filters_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                                        C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_parts_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "cph_parts_set_exact_threshold": (C.c_int, [C.c_void_p, C.c_uint64]),
    "cph_parts_filter_create_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "cph_parts_filter_destroy": (C.c_int, [C.c_void_p]),
    "cph_parts_last_search_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cph_parts_last_query_expansions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "cph_parts_num_parts": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "cph_parts_part": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "cph_parts_bounds": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cph_merge_rows_hook": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "cph_host_part_bounds": (C.c_int, [C.c_uint64, C.c_uint32, C.c_void_p]),
    "cph_encode_query": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_entry_point": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]),
    "cph_fastscan_block": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float,
                                     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_exact_l2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "cph_host_rewrite_index": (C.c_int, [C.c_char_p, C.c_char_p]),
    "cph_host_repack_block": (C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]),
    "cph_host_relayout_block": (C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_export_blocks": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]),
    "cph_host_encode_query": (C.c_int, [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_host_rows_filter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "cph_fastscan_stream_create": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64,
                                             C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "cph_fastscan_stream_run": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "cph_fastscan_stream_export": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.POINTER(C.c_float)]),
    "cph_fastscan_stream_eval": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "cph_fastscan_stream_destroy": (C.c_int, [C.c_void_p]),
    "cph_set_metric": (C.c_int, [C.c_void_p, C.c_int]),
    "cph_get_metric": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "cph_multi_set_metric": (C.c_int, [C.c_void_p, C.c_int]),
    "cph_parts_set_metric": (C.c_int, [C.c_void_p, C.c_int]),
    "cph_metric_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cph_normalize_rows_hook": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint64)]),
    "cph_host_normalize_rows": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint64)]),
    "cph_set_metric_ip": (C.c_int, [C.c_void_p]),
    "cph_multi_set_metric_ip": (C.c_int, [C.c_void_p]),
    "cph_set_ip_bound": (C.c_int, [C.c_void_p, C.c_float]),
    "cph_get_ip_bound": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "cph_multi_set_ip_bound": (C.c_int, [C.c_void_p, C.c_float]),
    "cph_multi_get_ip_bound": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "cph_ip_augment_hook": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                      C.POINTER(C.c_float), C.POINTER(C.c_uint64)]),
    "cph_ip_epilogue_hook": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_int]),
    "cph_host_ip_augment": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                      C.POINTER(C.c_float), C.POINTER(C.c_uint64)]),
    "cph_host_ip_epilogue": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "cph_rescore_vectors_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "cph_rescore_vectors_destroy": (C.c_int, [C.c_void_p]),
    "cph_rescore_vectors_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                           C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cph_rescore_vectors_get": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "cph_search_rescored": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                      C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_search_rescored_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                                             C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_multi_search_rescored": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                                            C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_debug_time_rescored": (C.c_int, [C.c_void_p, C.c_int]),
    "cph_debug_last_rescored_us": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "cph_rescore_rows_hook": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_host_rescore_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                        C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cph_host_rescore_rows_in": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                           C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
}
RESCORE_FLOAT16, RESCORE_FLOAT32 = 0, 1      # cph_rescore_vectors_create: dtype
RESCORE_L2, RESCORE_IP = 0, 1                # ... and metric

_LIB = None


def _share_hip_runtime_with_torch():
    """A PyTorch-ROCm wheel bundles its own libamdhip64 / libhsa-runtime64.  If this library pulled in the
    system copies first and torch were imported afterwards, the process would hold two HSA runtimes and torch
    would report "No HIP GPUs are available".  When torch is installed but not imported yet, load ITS HIP
    runtime first (same soname: our library then binds to it, exactly as it does when torch was imported
    first); torch itself is not imported."""
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """Loads (building if needed) the HIP library.  There is no fallback: if the library cannot
    be built or loaded the product path is unavailable and this raises."""
    global _LIB
    if _LIB is None:
        path = os.environ.get("CPH_LIB_PATH")  # diagnostic builds (e.g. -DCPH_PHASE_TIMERS)
        if not path:
            path = _build.LIB_PATH
            if _build.needs_build():
                path = _build.build_library()
        _share_hip_runtime_with_torch()
        L = C.CDLL(path)
        diagnostic = bool(os.environ.get("CPH_LIB_PATH"))
        for name, (res, args) in SYMBOLS.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                if diagnostic:          # an A/B build of an older tree may lack the newest test hooks
                    continue
                raise
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def check(rc):
    """Maps a cph_status to the exception type pybind11 raises for the reference
    (std::invalid_argument -> ValueError, std::runtime_error -> RuntimeError, bad_alloc ->
    MemoryError)."""
    if rc == OK:
        return
    msg = lib().cph_last_error().decode("utf-8", "replace")
    if rc == INVALID_ARGUMENT:
        raise ValueError(msg)
    if rc == OUT_OF_MEMORY:
        raise MemoryError(msg)
    if rc == NOT_IMPLEMENTED:
        raise NotImplementedError(msg)
    raise RuntimeError(msg)
