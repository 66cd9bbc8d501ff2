"""cphnsw_mi355x — MI355X-native query path of CP-HNSW behind the reference's Python API.

    from cphnsw_mi355x import CPIndex      # drop-in for `from cphnsw import CPIndex`
"""
from .index import (CPIndex, FastScanStream, GroupKeys, IdFilter, RescoreVectors, combine_filters, encode_edges, heap_ops_debug,  # noqa: F401
                    knn_bruteforce, knn_debug, pack_allowed_bits, select_layer_debug, select_neighbors_debug)

__all__ = ["CPIndex", "FastScanStream", "GroupKeys", "IdFilter", "RescoreVectors", "combine_filters", "encode_edges", "heap_ops_debug", "knn_bruteforce", "knn_debug",
           "pack_allowed_bits", "select_layer_debug", "select_neighbors_debug"]
