"""ctypes binding of the C ABI declared in include/em2_lsh.h (libem2lsh.so, built for gfx950).

This module is plumbing only: it loads the shared library that holds the HIP kernels and exposes numpy /
device-pointer level wrappers.  There is no Python or CPU implementation of the path behind it: if the
library is missing or no GPU is visible the calls raise RuntimeError.
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIBRARY_PATH = os.environ.get("EM2_LIBRARY") or os.path.join(_HERE, "libem2lsh.so")   # override: A/B builds only
CSRC_DIR = os.path.join(_HERE, "csrc")

# std::pair<CellId,float> (src/SimilarPairs.hpp:53-56) and std::pair<GeneId,float> (src/ExpressionMatrixSubset.hpp:36)
PAIR_DTYPE = np.dtype([("cell", "<u4"), ("similarity", "<f4")])
COUNT_DTYPE = np.dtype([("gene", "<u4"), ("count", "<f4")])

EM2_OK = 0
EM2_ERROR_INVALID_ARGUMENT = 1
EM2_ERROR_NO_DEVICE = 2
EM2_ERROR_UNSUPPORTED = 6

_lib = None

# name -> (restype, argtypes); every symbol include/em2_lsh.h declares.
_c = ctypes
SYMBOLS = {
    "em2_abi_version": (_c.c_int, []),
    "em2_last_error": (_c.c_char_p, []),
    "em2_lsh_generate_vectors": (_c.c_int, [_c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_void_p]),
    "em2_lsh_similarity_table": (_c.c_int, [_c.c_uint32, _c.c_void_p]),
    "em2_murmur_hash_64a": (_c.c_uint64, [_c.c_void_p, _c.c_int, _c.c_uint64]),
    "em2_device_count": (_c.c_int, [_c.POINTER(_c.c_int)]),
    "em2_set_device": (_c.c_int, [_c.c_int]),
    "em2_compute_signatures": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_void_p,
                                          _c.c_uint32, _c.c_void_p]),
    "em2_find_similar_pairs4": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_double,
                                           _c.c_void_p, _c.c_void_p]),
    "em2_find_similar_pairs5": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_double,
                                           _c.c_uint32, _c.c_uint64, _c.c_void_p, _c.c_void_p]),
    "em2_dev_compute_signatures_workspace": (_c.c_size_t, [_c.c_uint32, _c.c_uint32]),
    "em2_dev_compute_signatures": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_void_p,
                                              _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_size_t,
                                              _c.c_void_p]),
    "em2_dev_compute_signatures_tier": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_int, _c.c_void_p]),
    "em2_dev_compute_signatures_listed": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_int, _c.c_void_p]),
    "em2_dev_vector_aux_bytes": (_c.c_size_t, [_c.c_uint32, _c.c_uint32]),
    "em2_dev_prepare_vectors": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_void_p, _c.c_void_p]),
    "em2_dev_find_similar_pairs4_workspace": (_c.c_size_t, [_c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32]),
    "em2_dev_find_similar_pairs4": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32,
                                               _c.c_uint32, _c.c_double, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                               _c.c_size_t, _c.c_void_p]),
    "em2_find_similar_pairs0": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_double,
                                           _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "em2_dev_find_similar_pairs0_workspace": (_c.c_size_t, [_c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32]),
    "em2_dev_find_similar_pairs0": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32,
                                               _c.c_uint32, _c.c_double, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                               _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "em2_matrix_find_similar_pairs0": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_char_p, _c.c_size_t,
                                                  _c.c_double]),
    "em2_find_similar_gene_pairs0": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_int, _c.c_uint32,
                                                _c.c_double, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "em2_set_gene_pairs_buffer_mb": (None, [_c.c_uint64]),
    "em2_gene_information_content": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_void_p, _c.c_void_p,
                                                _c.c_void_p, _c.c_void_p]),
    "em2_dev_gene_information_content_workspace": (_c.c_size_t, [_c.c_uint32, _c.c_uint32, _c.c_uint64]),
    "em2_dev_gene_information_content": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_uint64, _c.c_void_p,
                                                    _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "em2_set_gene_information_max_blocks": (None, [_c.c_uint32]),
    "em2_rank_genes": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_void_p,
                                  _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "em2_dev_rank_genes_workspace": (_c.c_size_t, [_c.c_uint32, _c.c_uint32, _c.c_uint64, _c.c_uint32]),
    "em2_dev_rank_genes": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_uint64, _c.c_void_p, _c.c_void_p,
                                      _c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t,
                                      _c.c_void_p]),
    "em2_set_rank_genes_test_limits": (None, [_c.c_uint32, _c.c_uint32, _c.c_uint32]),
    "em2_matrix_rank_genes": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_int, _c.c_void_p, _c.c_uint32, _c.c_void_p,
                                         _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "em2_cell_norm_inverses": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_void_p, _c.c_void_p]),
    "em2_matrix_gene_information_content": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_int, _c.c_void_p]),
    "em2_matrix_create_gene_set_using_information_content": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_int,
                                                                        _c.c_double, _c.c_char_p]),
    "em2_matrix_create_well_expressed_gene_set": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_char_p, _c.c_uint32]),
    "em2_matrix_remove_gene_set": (_c.c_int, [_c.c_void_p, _c.c_char_p]),
    "em2_tool_add_cells": (_c.c_int, [_c.c_char_p, _c.c_void_p, _c.c_void_p, _c.c_uint32]),
    "em2_matrix_find_similar_gene_pairs0": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_int, _c.c_char_p,
                                                       _c.c_size_t, _c.c_double]),
    "em2_matrix_remove_similar_gene_pairs": (_c.c_int, [_c.c_void_p, _c.c_char_p]),
    "em2_similar_gene_pairs_write": (_c.c_int, [_c.c_char_p, _c.c_char_p, _c.c_char_p, _c.c_char_p, _c.c_size_t, _c.c_int,
                                                _c.c_uint32, _c.c_void_p, _c.c_void_p]),
    "em2_similar_gene_pairs_read": (_c.c_int, [_c.c_char_p, _c.c_char_p, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64),
                                               _c.POINTER(_c.c_int), _c.c_char_p, _c.c_char_p, _c.POINTER(_c.c_uint64),
                                               _c.POINTER(_c.c_uint64), _c.c_void_p, _c.c_void_p]),
    "em2_analyze_similar_pairs": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_void_p, _c.c_void_p,
                                             _c.c_uint32, _c.c_void_p, _c.c_double, _c.c_char_p, _c.c_char_p, _c.c_void_p,
                                             _c.c_void_p, _c.c_void_p]),
    "em2_matrix_analyze_similar_pairs": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_double, _c.c_char_p]),
    "em2_matrix_compute_cell_similarity": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_uint32, _c.c_uint32, _c.c_void_p]),
    "em2_matrix_compare_similar_pairs": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_char_p]),
    "em2_find_similar_pairs6": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_double, _c.c_uint32,
                                           _c.c_uint32, _c.c_uint32, _c.c_int32, _c.c_void_p, _c.c_void_p]),
    "em2_dev_find_similar_pairs6": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32,
                                               _c.c_double, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_int32,
                                               _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "em2_matrix_find_similar_pairs6": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_char_p, _c.c_char_p,
                                                  _c.c_size_t, _c.c_double, _c.c_size_t, _c.c_size_t, _c.c_size_t,
                                                  _c.c_int]),
    "em2_find_similar_pairs7": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_double, _c.c_void_p,
                                           _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_void_p, _c.c_void_p]),
    "em2_dev_find_similar_pairs7": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32,
                                               _c.c_double, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_uint32,
                                               _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "em2_matrix_find_similar_pairs7": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_char_p, _c.c_char_p,
                                                  _c.c_size_t, _c.c_double, _c.c_void_p, _c.c_uint32, _c.c_uint32,
                                                  _c.c_size_t]),
    "em2_dev_subset_workspace": (_c.c_size_t, [_c.c_uint32]),
    "em2_dev_subset_count": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_uint32,
                                        _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "em2_dev_subset_fill": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_uint32,
                                       _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "em2_subset_find_similar_pairs4": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_uint32,
                                                  _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_void_p, _c.c_uint32,
                                                  _c.c_void_p, _c.c_uint32, _c.c_double, _c.c_void_p, _c.c_void_p]),
    "em2_cell_graph_label_propagation": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                                    _c.c_uint64, _c.c_uint64, _c.c_uint64, _c.c_uint64, _c.c_void_p,
                                                    _c.c_void_p]),
    "em2_dev_cell_graph_label_propagation": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                                        _c.c_uint64, _c.c_uint64, _c.c_uint64, _c.c_uint64, _c.c_void_p,
                                                        _c.c_void_p]),
    "em2_cluster_average_expression": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_void_p, _c.c_void_p,
                                                  _c.c_uint32, _c.c_void_p]),
    "em2_cluster_similarities": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_uint64,
                                            _c.c_void_p]),
    "em2_cluster_graph_create": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_void_p, _c.c_uint32,
                                            _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_uint64,
                                            _c.c_double, _c.c_double, _c.POINTER(_c.c_void_p)]),
    "em2_cluster_graph_sizes": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_uint32),
                                           _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    "em2_cluster_graph_get": (_c.c_int, [_c.c_void_p] * 9),
    "em2_cluster_graph_facts": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32]),
    "em2_cluster_graph_free": (None, [_c.c_void_p]),
    "em2_signature_graph_create": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_uint64, _c.POINTER(_c.c_void_p)]),
    "em2_dev_signature_graph_create": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_uint64, _c.POINTER(_c.c_void_p)]),
    "em2_signature_graph_sizes": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_uint32),
                                             _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    "em2_signature_graph_get": (_c.c_int, [_c.c_void_p] * 6),
    "em2_signature_graph_free": (None, [_c.c_void_p]),
    "em2_lsh_signature_statistics": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_void_p]),
    "em2_dev_lsh_signature_statistics": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_void_p]),
    "em2_analyze_lsh_signatures": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_char_p]),
    "em2_matrix_create_signature_graph": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_uint64, _c.POINTER(_c.c_void_p)]),
    "em2_matrix_analyze_lsh_signatures": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_size_t, _c.c_uint, _c.c_char_p]),
    "em2_gene_graph_create": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_uint32,
                                         _c.c_double, _c.c_uint64, _c.POINTER(_c.c_void_p)]),
    "em2_dev_gene_graph_create": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_uint32,
                                             _c.c_double, _c.c_uint64, _c.POINTER(_c.c_void_p)]),
    "em2_gene_graph_sizes": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint32)]),
    "em2_gene_graph_get": (_c.c_int, [_c.c_void_p] * 8),
    "em2_gene_graph_free": (None, [_c.c_void_p]),
    "em2_graph_layout": (_c.c_int, [_c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "em2_dev_graph_layout": (_c.c_int, [_c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                        _c.c_void_p]),
    "em2_graph_layout_forces": (_c.c_int, [_c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_double, _c.c_void_p, _c.c_void_p,
                                           _c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_double)]),
    "em2_graph_layout_pyramid": (_c.c_int, [_c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint32, _c.c_void_p,
                                            _c.c_void_p, _c.c_void_p]),
    "em2_dev_graph_layout_pyramid": (_c.c_int, [_c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint32, _c.c_void_p,
                                                _c.c_void_p, _c.c_void_p]),
    "em2_graph_layout_forces_pyramid": (_c.c_int, [_c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_double, _c.c_uint32, _c.c_void_p,
                                                   _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_double)]),
    "em2_graph_layout_multilevel": (_c.c_int, [_c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint32, _c.c_void_p,
                                               _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "em2_dev_graph_layout_multilevel": (_c.c_int, [_c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint32,
                                                   _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "em2_graph_layout_coarsen": (_c.c_int, [_c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_uint32,
                                            _c.c_uint32, _c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_uint32),
                                            _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_uint64)]),
    "em2_graph_layout_forces_weighted": (_c.c_int, [_c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64,
                                                    _c.c_double, _c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                                    _c.POINTER(_c.c_double)]),
    "em2_matrix_create_gene_graph": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_int64, _c.c_double, _c.POINTER(_c.c_void_p)]),
    "em2_matrix_create_gene_set_intersection": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.POINTER(_c.c_int)]),
    "em2_matrix_create_gene_set_union": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.POINTER(_c.c_int)]),
    "em2_matrix_create_gene_set_difference": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_char_p, _c.POINTER(_c.c_int)]),
    "em2_dev_dense_expression_workspace": (_c.c_size_t, [_c.c_uint32]),
    "em2_dev_dense_expression": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_uint32, _c.c_uint32,
                                            _c.c_int, _c.c_uint32, _c.c_uint32, _c.c_int, _c.c_void_p, _c.c_uint64, _c.c_void_p,
                                            _c.c_size_t, _c.c_void_p]),
    "em2_dense_expression": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_uint32,
                                        _c.c_uint32, _c.c_int, _c.c_int, _c.c_void_p, _c.c_uint64]),
    "em2_matrix_dense_expression": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_int, _c.c_int, _c.c_uint32, _c.c_uint32,
                                               _c.c_void_p]),
    "em2_dev_cell_similarities_to_cell_workspace": (_c.c_size_t, [_c.c_uint32, _c.c_uint32]),
    "em2_cell_similarities_row_in_lds": (_c.c_int, [_c.c_uint32]),
    "em2_dev_cell_similarities_to_cell": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_uint32, _c.c_uint32,
                                                     _c.c_uint32, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_size_t,
                                                     _c.c_void_p]),
    "em2_cell_similarities_to_cell": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_uint32, _c.c_uint32,
                                                 _c.c_uint32, _c.c_void_p, _c.c_uint32, _c.c_void_p]),
    "em2_matrix_cell_similarities_to_cell": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_uint32, _c.c_void_p, _c.c_uint32, _c.c_void_p]),
    "em2_dev_gene_expression_of_cells_workspace": (_c.c_size_t, []),
    "em2_dev_gene_expression_of_cells": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_uint32, _c.c_uint32,
                                                    _c.c_uint32, _c.c_int, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_void_p,
                                                    _c.c_size_t, _c.c_void_p]),
    "em2_gene_expression_of_cells": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_uint32, _c.c_uint32,
                                                _c.c_uint32, _c.c_int, _c.c_void_p, _c.c_uint32, _c.c_void_p]),
    "em2_matrix_gene_expression_of_cells": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_uint32, _c.c_int, _c.c_void_p, _c.c_uint32,
                                                       _c.c_void_p]),
    "em2_dev_spectral_colors_workspace": (_c.c_size_t, []),
    "em2_dev_spectral_colors": (_c.c_int, [_c.c_void_p, _c.c_uint64, _c.c_double, _c.c_double, _c.c_int, _c.c_int, _c.c_void_p,
                                           _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "em2_spectral_colors": (_c.c_int, [_c.c_void_p, _c.c_uint64, _c.c_double, _c.c_double, _c.c_int, _c.c_int, _c.c_void_p,
                                       _c.c_void_p]),
    "em2_meta_data_number": (_c.c_int, [_c.c_char_p, _c.c_uint64, _c.POINTER(_c.c_double)]),
    "em2_graph_draw_long_edge_steps": (_c.c_uint32, []),
    "em2_dev_graph_draw_workspace": (_c.c_size_t, [_c.c_uint32, _c.c_uint64]),
    "em2_dev_graph_draw": (_c.c_int, [_c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_int,
                                      _c.c_uint32, _c.c_double, _c.c_double, _c.c_double, _c.c_double, _c.c_void_p, _c.c_void_p,
                                      _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "em2_graph_draw": (_c.c_int, [_c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_uint32,
                                  _c.c_double, _c.c_double, _c.c_double, _c.c_double, _c.c_void_p, _c.c_void_p]),
    "em2_dev_graph_compose": (_c.c_int, [_c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_void_p]),
    "em2_graph_compose": (_c.c_int, [_c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_void_p]),
    "em2_graph_write_svg": (_c.c_int, [_c.c_char_p, _c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p,
                                       _c.c_void_p, _c.c_int, _c.c_double, _c.c_double, _c.c_double, _c.c_double, _c.c_double,
                                       _c.c_double, _c.c_char_p, _c.c_uint64, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_char_p,
                                       _c.c_uint64, _c.c_char_p]),
    "em2_pie_census_wave_cells": (_c.c_uint32, []),
    "em2_pie_census_create": (_c.c_int, [_c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint32, _c.c_void_p,
                                         _c.c_uint32, _c.POINTER(_c.c_void_p)]),
    "em2_dev_pie_census": (_c.c_int, [_c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint32, _c.c_void_p,
                                      _c.c_uint32, _c.POINTER(_c.c_void_p)]),
    "em2_matrix_pie_census": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint32,
                                         _c.c_char_p, _c.POINTER(_c.c_void_p)]),
    "em2_pie_census_sizes": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint32)]),
    "em2_pie_census_get": (_c.c_int, [_c.c_void_p] * 5),
    "em2_pie_census_values_sizes": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    "em2_pie_census_values_get": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "em2_pie_census_free": (None, [_c.c_void_p]),
    "em2_order_by_count": (_c.c_int, [_c.c_void_p, _c.c_uint64, _c.c_void_p]),
    "em2_signature_graph_random_colors": (_c.c_int, [_c.c_uint32, _c.c_void_p]),
    "em2_graph_draw_pies_wave_radius": (_c.c_double, []),
    "em2_dev_graph_draw_pies_workspace": (_c.c_size_t, [_c.c_uint32, _c.c_uint64]),
    "em2_dev_graph_draw_pies": (_c.c_int, [_c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p,
                                           _c.c_int, _c.c_uint32, _c.c_double, _c.c_double, _c.c_double, _c.c_void_p, _c.c_uint64,
                                           _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                           _c.c_size_t, _c.c_void_p]),
    "em2_graph_draw_pies": (_c.c_int, [_c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p,
                                       _c.c_int, _c.c_uint32, _c.c_double, _c.c_double, _c.c_double, _c.c_void_p, _c.c_uint64,
                                       _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "em2_pie_boundaries": (_c.c_int, [_c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "em2_signature_graph_write_svg": (_c.c_int, [_c.c_char_p, _c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64,
                                                 _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_double, _c.c_double, _c.c_double,
                                                 _c.c_double, _c.c_double, _c.c_double, _c.c_void_p, _c.c_char_p, _c.c_uint64,
                                                 _c.c_void_p, _c.c_void_p]),
    "em2_matrix_cell_expression_counts": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.POINTER(_c.c_uint64), _c.c_void_p]),
    "em2_matrix_create_cell_set": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_void_p, _c.c_uint32]),
    "em2_matrix_create_cell_set_intersection": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p]),
    "em2_matrix_create_cell_set_union": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p]),
    "em2_matrix_create_cell_set_difference": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_char_p]),
    "em2_matrix_downsample_cell_set": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_double, _c.c_int]),
    "em2_matrix_remove_cell_set": (_c.c_int, [_c.c_void_p, _c.c_char_p]),
    "em2_matrix_cell_set_names": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint64), _c.c_void_p]),
    "em2_analyze_lsh": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_void_p, _c.c_uint32, _c.c_void_p,
                                   _c.c_uint32, _c.c_double, _c.c_char_p, _c.c_char_p, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                   _c.c_void_p, _c.c_void_p]),
    "em2_matrix_analyze_lsh": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_size_t, _c.c_uint, _c.c_double,
                                          _c.c_char_p]),
    "em2_dist_find_similar_pairs4_workspace": (_c.c_size_t, [_c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32]),
    "em2_dist_find_similar_pairs4_form": (_c.c_int, [_c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32]),
    "em2_dist_find_similar_pairs4": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_double,
                                                _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p,
                                                _c.c_void_p]),
    "em2_dist_find_similar_pairs4_with": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_double,
                                                     _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p,
                                                     _c.c_void_p]),
    "em2_dev_find_similar_pairs4_form": (_c.c_int, [_c.c_uint32, _c.c_uint32]),
    "em2_dev_find_similar_pairs4_form_for": (_c.c_int, [_c.c_uint32, _c.c_uint32, _c.c_uint32]),
    "em2_dev_find_similar_pairs4_last_launch": (_c.c_int, [_c.c_void_p, _c.c_uint32]),
    "em2_dev_find_similar_pairs5_last_launch": (_c.c_int, [_c.c_void_p, _c.c_uint32]),
    "em2_dev_release_scratch": (None, []),
    "em2_dev_fsp4_sharded_plan": (_c.c_int, [_c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32,
                                             _c.c_void_p, _c.c_uint32]),
    "em2_dev_fsp4_sharded_phase": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_double,
                                              _c.c_uint32, _c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                              _c.c_size_t, _c.c_uint64, _c.c_void_p]),
    "em2_dev_fsp4_sharded_status": (_c.c_int, [_c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_void_p,
                                               _c.c_void_p, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint32)]),
    "em2_dev_find_similar_pairs4_status": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_void_p]),
    "em2_dev_find_similar_pairs5": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32,
                                               _c.c_uint32, _c.c_double, _c.c_uint32, _c.c_uint64, _c.c_void_p,
                                               _c.c_void_p, _c.c_void_p]),
    "em2_matrix_open": (_c.c_int, [_c.c_char_p, _c.POINTER(_c.c_void_p)]),
    "em2_matrix_close": (None, [_c.c_void_p]),
    "em2_matrix_find_similar_pairs4": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_char_p, _c.c_size_t,
                                                  _c.c_double, _c.c_size_t, _c.c_uint]),
    "em2_matrix_compute_lsh_signatures": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_char_p,
                                                     _c.c_size_t, _c.c_uint]),
    "em2_matrix_find_similar_pairs5": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_char_p, _c.c_char_p,
                                                  _c.c_size_t, _c.c_double, _c.c_size_t, _c.c_size_t]),
    "em2_matrix_remove_similar_pairs": (_c.c_int, [_c.c_void_p, _c.c_char_p]),
    "em2_matrix_subset": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.POINTER(_c.c_uint32),
                                     _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_uint64), _c.c_void_p, _c.c_void_p]),
    "em2_similar_pairs_write": (_c.c_int, [_c.c_char_p, _c.c_char_p, _c.c_char_p, _c.c_char_p, _c.c_size_t,
                                           _c.c_uint32, _c.c_void_p, _c.c_void_p]),
    "em2_similar_pairs_read": (_c.c_int, [_c.c_char_p, _c.c_char_p, _c.POINTER(_c.c_uint64),
                                          _c.POINTER(_c.c_uint64), _c.c_void_p, _c.c_void_p]),
    "em2_similar_pairs_info": (_c.c_int, [_c.c_char_p, _c.c_char_p, _c.POINTER(_c.c_uint64),
                                          _c.POINTER(_c.c_uint64), _c.c_char_p, _c.c_char_p]),
    "em2_matrix_cell_set": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.POINTER(_c.c_uint32), _c.c_void_p]),
    "em2_matrix_gene_set": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.POINTER(_c.c_uint32), _c.c_void_p]),
    "em2_cell_graph_edges": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_void_p,
                                        _c.c_void_p, _c.c_uint32, _c.c_double, _c.c_uint32, _c.c_void_p,
                                        _c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_uint64)]),
    "em2_dev_cell_graph_edges": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint32, _c.c_void_p,
                                            _c.c_void_p, _c.c_uint32, _c.c_double, _c.c_uint32, _c.c_void_p,
                                            _c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_uint64)]),
    "em2_lsh_write": (_c.c_int, [_c.c_char_p, _c.c_char_p, _c.c_uint64, _c.c_uint64, _c.c_void_p]),
    "em2_lsh_read": (_c.c_int, [_c.c_char_p, _c.c_char_p, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64),
                                _c.c_void_p]),
    "em2_tool_create_directory": (_c.c_int, [_c.c_char_p, _c.c_uint32, _c.c_uint32, _c.c_void_p, _c.c_void_p]),
    "em2_tool_add_gene_set": (_c.c_int, [_c.c_char_p, _c.c_char_p, _c.c_void_p, _c.c_uint32]),
    "em2_tool_add_cell_set": (_c.c_int, [_c.c_char_p, _c.c_char_p, _c.c_void_p, _c.c_uint32]),
    "em2_contingency_create": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_uint32, _c.c_uint32, _c.c_int,
                                          _c.POINTER(_c.c_void_p)]),
    "em2_dev_contingency": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_uint32, _c.c_uint32, _c.c_int,
                                       _c.POINTER(_c.c_void_p)]),
    "em2_contingency_sizes": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_uint64),
                                         _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_int)]),
    "em2_contingency_get": (_c.c_int, [_c.c_void_p] * 7),
    "em2_contingency_free": (None, [_c.c_void_p]),
    "em2_rand_index": (_c.c_int, [_c.c_uint64, _c.c_uint64, _c.c_uint64, _c.c_uint64, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
    "em2_cell_graph_compare": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64] * 2 +
                                         [_c.c_int, _c.POINTER(_c.c_void_p)]),
    "em2_dev_cell_graph_compare": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64] * 2 +
                                             [_c.c_int, _c.POINTER(_c.c_void_p)]),
    "em2_graph_comparison_sizes": (_c.c_int, [_c.c_void_p] + [_c.POINTER(_c.c_uint64)] * 6 + [_c.POINTER(_c.c_int)]),
    "em2_graph_comparison_get": (_c.c_int, [_c.c_void_p] * 3),
    "em2_graph_comparison_free": (None, [_c.c_void_p]),
    "em2_graph_group_colors": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_int,
                                          _c.POINTER(_c.c_void_p)]),
    "em2_dev_graph_group_colors": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_int,
                                              _c.POINTER(_c.c_void_p)]),
    "em2_group_colors_sizes": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_int)]),
    "em2_group_colors_get": (_c.c_int, [_c.c_void_p] * 5),
    "em2_group_colors_free": (None, [_c.c_void_p]),
    "em2_matrix_set_cell_meta_data": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_char_p, _c.c_char_p]),
    "em2_matrix_get_cell_meta_data_value": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_char_p, _c.POINTER(_c.c_uint64), _c.c_void_p]),
    "em2_matrix_get_cell_meta_data": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.POINTER(_c.c_uint64), _c.c_void_p]),
    "em2_matrix_remove_cell_meta_data": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p]),
    "em2_matrix_create_cell_set_using_meta_data": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_char_p, _c.c_int]),
    "em2_matrix_compute_meta_data_rand_index": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_char_p,
                                                           _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
    "em2_matrix_meta_data_table": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_char_p, _c.POINTER(_c.c_void_p)]),
    "em2_meta_data_table_sizes": (_c.c_int, [_c.c_void_p] + [_c.POINTER(_c.c_uint64)] * 5 + [_c.POINTER(_c.c_int)]),
    "em2_meta_data_table_get": (_c.c_int, [_c.c_void_p] * 9),
    "em2_meta_data_table_cell_rows": (_c.c_int, [_c.c_void_p, _c.c_void_p]),
    "em2_meta_data_table_free": (None, [_c.c_void_p]),
    "em2_matrix_flush": (_c.c_int, [_c.c_void_p]),
    "em2_tool_create_meta_data": (_c.c_int, [_c.c_char_p, _c.c_uint32, _c.c_uint64, _c.c_uint64]),
    "em2_matrix_create": (_c.c_int, [_c.c_char_p, _c.POINTER(_c.c_void_p)]),
    "em2_matrix_gene_count": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint32)]),
    "em2_matrix_cell_count": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint32)]),
    "em2_matrix_add_gene": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.POINTER(_c.c_int)]),
    "em2_matrix_gene_name": (_c.c_int, [_c.c_void_p, _c.c_uint32, _c.POINTER(_c.c_uint64), _c.c_void_p]),
    "em2_matrix_gene_id_from_name": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.POINTER(_c.c_uint32)]),
    "em2_matrix_cell_id_from_string": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.POINTER(_c.c_uint32)]),
    "em2_matrix_add_cell": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_uint64, _c.c_uint32, _c.c_char_p, _c.c_uint64, _c.c_void_p,
                                       _c.c_uint32, _c.POINTER(_c.c_uint32)]),
    "em2_dev_ingest_count": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_uint32,
                                        _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "em2_dev_ingest_fill": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_uint32,
                                       _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "em2_set_ingest_lds_row_limit": (None, [_c.c_uint32]),
    "em2_matrix_add_cells_csr": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_uint64, _c.c_uint32, _c.c_char_p, _c.c_uint64, _c.c_uint32,
                                            _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_char_p, _c.c_char_p,
                                            _c.c_uint64, _c.c_uint32, _c.c_uint64, _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_uint32)]),
    "em2_csv_tokenize": (_c.c_int, [_c.c_char_p, _c.c_char_p, _c.c_uint64, _c.c_int, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64),
                                    _c.c_void_p]),
    "em2_dev_csv_parse": (_c.c_int, [_c.c_void_p, _c.c_uint64, _c.c_char_p, _c.c_uint32, _c.c_uint32, _c.c_void_p, _c.c_uint32, _c.c_uint32,
                                     _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "em2_set_csv_tile_bytes": (None, [_c.c_uint32]),
    "em2_matrix_add_cells_csv": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_char_p, _c.c_char_p, _c.c_char_p, _c.c_char_p, _c.c_uint64,
                                            _c.c_uint32, _c.c_uint64, _c.c_int, _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_uint32),
                                            _c.POINTER(_c.c_uint64)]),
    "em2_matrix_add_cell_meta_data_csv": (_c.c_int, [_c.c_void_p, _c.c_char_p]),
}


def build_library(verbose=False):
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    result = subprocess.run(["make", "-C", CSRC_DIR, "-j4"], capture_output=True, text=True)
    if verbose or result.returncode != 0:
        print(result.stdout)
        print(result.stderr)
    if result.returncode != 0:
        raise RuntimeError("building libem2lsh.so failed:\n" + result.stderr[-4000:])
    return LIBRARY_PATH


def _share_hip_runtime_with_torch():
    """torch wheels bundle their own libamdhip64.so.  Two HIP runtimes in one process cannot both see the GPU,
    and the only load order that works is torch first (libem2lsh.so then binds to the runtime torch mapped,
    same SONAME).  So when torch is installed, import it before mapping libem2lsh.so.  torch stays plumbing:
    nothing of it is called here."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        if importlib.util.find_spec("torch") is not None:
            import torch  # noqa: F401
    except Exception:
        pass


def load():
    """Load libem2lsh.so.  Raises RuntimeError (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    _share_hip_runtime_with_torch()
    if not os.path.exists(LIBRARY_PATH):
        raise RuntimeError(
            "%s is missing: run `make -C %s` (or __graft_entry__.build()). "
            "There is no fallback implementation." % (LIBRARY_PATH, CSRC_DIR))
    lib = ctypes.CDLL(LIBRARY_PATH)
    for name, (restype, argtypes) in SYMBOLS.items():
        fn = getattr(lib, name)       # AttributeError here == the library does not export a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def last_error():
    message = load().em2_last_error()
    return message.decode("utf-8", "replace") if message else ""


def check(rc):
    if rc != EM2_OK:
        raise RuntimeError(last_error() or ("em2 error %d" % rc))


def word_count(lsh_count):
    return (int(lsh_count) - 1) // 64 + 1


def _ptr(array):
    return array.ctypes.data_as(ctypes.c_void_p)


def device_count():
    n = ctypes.c_int(0)
    check(load().em2_device_count(ctypes.byref(n)))
    return n.value


def lsh_generate_vectors(gene_count, lsh_count, seed):
    """Lsh::generateLshVectors (src/Lsh.cpp:68-113) -> float64 [gene_count, lsh_count]."""
    out = np.empty((gene_count, lsh_count), dtype=np.float64)
    check(load().em2_lsh_generate_vectors(gene_count, lsh_count, seed, _ptr(out)))
    return out


def similarity_table(lsh_count):
    out = np.empty(lsh_count + 1, dtype=np.float64)
    check(load().em2_lsh_similarity_table(lsh_count, _ptr(out)))
    return out


def murmur_hash_64a(data, seed=231):
    buf = np.ascontiguousarray(data).view(np.uint8)
    return int(load().em2_murmur_hash_64a(_ptr(buf), buf.size, seed))


def make_counts(genes, counts):
    data = np.empty(len(genes), dtype=COUNT_DTYPE)
    data["gene"] = genes
    data["count"] = counts
    return data


def compute_signatures(toc, data, gene_count, vectors, lsh_count):
    """Host-buffer Lsh::computeCellLshSignatures (src/Lsh.cpp:118-224) on the GPU -> uint64 [cells, words]."""
    toc = np.ascontiguousarray(toc, dtype=np.uint64)
    data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
    vectors = np.ascontiguousarray(vectors, dtype=np.float64)
    cell_count = len(toc) - 1
    assert vectors.shape == (gene_count, lsh_count)
    out = np.zeros((cell_count, word_count(lsh_count)), dtype=np.uint64)
    check(load().em2_compute_signatures(_ptr(toc), _ptr(data), cell_count, gene_count, _ptr(vectors), lsh_count,
                                        _ptr(out)))
    return out


def find_similar_pairs4(signatures, lsh_count, k=100, similarity_threshold=0.2):
    """Host-buffer findSimilarPairs4 pair loop (src/ExpressionMatrixLsh.cpp:200-285) on the GPU.
    Returns (pairs[cells, k] of PAIR_DTYPE, used_count[cells])."""
    signatures = np.ascontiguousarray(signatures, dtype=np.uint64)
    cell_count = signatures.shape[0]
    assert signatures.shape[1] == word_count(lsh_count)
    pairs = np.zeros((cell_count, k), dtype=PAIR_DTYPE)
    used = np.zeros(cell_count, dtype=np.uint32)
    check(load().em2_find_similar_pairs4(_ptr(signatures), cell_count, lsh_count, k, similarity_threshold,
                                         _ptr(pairs), _ptr(used)))
    return pairs, used


def find_similar_pairs5(signatures, lsh_count, k, similarity_threshold, lsh_slice_length, bucket_overflow=1000):
    signatures = np.ascontiguousarray(signatures, dtype=np.uint64)
    cell_count = signatures.shape[0]
    pairs = np.zeros((cell_count, k), dtype=PAIR_DTYPE)
    used = np.zeros(cell_count, dtype=np.uint32)
    check(load().em2_find_similar_pairs5(_ptr(signatures), cell_count, lsh_count, k, similarity_threshold,
                                         lsh_slice_length, bucket_overflow, _ptr(pairs), _ptr(used)))
    return pairs, used


def cell_graph_edges(pairs, used_count, similar_pairs_cell_set, graph_cell_set, similarity_threshold,
                     max_connectivity):
    """CellGraph::CellGraph (src/CellGraph.cpp:33-117) -> (vertex0, vertex1, similarity) per edge, in the order
    the reference adds them; vertex v is graph_cell_set[v]."""
    pairs = np.ascontiguousarray(pairs, dtype=PAIR_DTYPE)
    used_count = np.ascontiguousarray(used_count, dtype=np.uint32)
    sp_cells = np.ascontiguousarray(similar_pairs_cell_set, dtype=np.uint32)
    graph_cells = np.ascontiguousarray(graph_cell_set, dtype=np.uint32)
    cell_count = len(used_count)
    k = pairs.shape[1] if pairs.ndim == 2 else 0
    if len(sp_cells) != cell_count or (pairs.ndim == 2 and pairs.shape[0] != cell_count):
        raise ValueError("pairs, used_count and the SimilarPairs cell set must describe the same cells")
    per_vertex = k if (max_connectivity == 0 or max_connectivity > k) else int(max_connectivity)
    capacity = max(1, len(graph_cells) * per_vertex)
    v0 = np.zeros(capacity, dtype=np.uint32)
    v1 = np.zeros(capacity, dtype=np.uint32)
    sim = np.zeros(capacity, dtype=np.float32)
    count = ctypes.c_uint64(0)
    check(load().em2_cell_graph_edges(_ptr(pairs), _ptr(used_count), cell_count, k, _ptr(sp_cells), _ptr(graph_cells),
                                      len(graph_cells), similarity_threshold, min(int(max_connectivity), 0xffffffff),
                                      _ptr(v0), _ptr(v1), _ptr(sim), ctypes.byref(count)))
    n = int(count.value)
    return v0[:n].copy(), v1[:n].copy(), sim[:n].copy()


def dev_cell_graph_edges(pairs_ptr, used_ptr, cell_count, k, similar_pairs_cell_set, graph_cell_set, similarity_threshold,
                         max_connectivity):
    """cell_graph_edges with the SimilarPairs content still on the device (device pointers as
    dev_find_similar_pairs4 left them); cell sets in, edges out as host arrays."""
    sp_cells = np.ascontiguousarray(similar_pairs_cell_set, dtype=np.uint32)
    graph_cells = np.ascontiguousarray(graph_cell_set, dtype=np.uint32)
    per_vertex = k if (max_connectivity == 0 or max_connectivity > k) else int(max_connectivity)
    capacity = max(1, len(graph_cells) * per_vertex)
    v0 = np.zeros(capacity, dtype=np.uint32)
    v1 = np.zeros(capacity, dtype=np.uint32)
    sim = np.zeros(capacity, dtype=np.float32)
    count = ctypes.c_uint64(0)
    check(load().em2_dev_cell_graph_edges(pairs_ptr, used_ptr, cell_count, k, _ptr(sp_cells), _ptr(graph_cells),
                                          len(graph_cells), similarity_threshold, min(int(max_connectivity), 0xffffffff),
                                          _ptr(v0), _ptr(v1), _ptr(sim), ctypes.byref(count)))
    n = int(count.value)
    return v0[:n].copy(), v1[:n].copy(), sim[:n].copy()


def dev_cell_graph_edges_to_device(pairs_ptr, used_ptr, cell_count, k, similar_pairs_cell_set, graph_cell_set, similarity_threshold,
                                   max_connectivity, v0_ptr, v1_ptr, sim_ptr):
    """dev_cell_graph_edges with the three edge arrays in DEVICE memory (pointers; room for
    len(graph_cell_set) * min(max_connectivity or k, k) edges each); returns the number of edges."""
    sp_cells = np.ascontiguousarray(similar_pairs_cell_set, dtype=np.uint32)
    graph_cells = np.ascontiguousarray(graph_cell_set, dtype=np.uint32)
    count = ctypes.c_uint64(0)
    check(load().em2_dev_cell_graph_edges(pairs_ptr, used_ptr, cell_count, k, _ptr(sp_cells), _ptr(graph_cells),
                                          len(graph_cells), similarity_threshold, min(int(max_connectivity), 0xffffffff),
                                          v0_ptr, v1_ptr, sim_ptr, ctypes.byref(count)))
    return int(count.value)


def dev_cell_graph_label_propagation(vertex_cell_ids, v0_ptr, v1_ptr, sim_ptr, edge_count, seed=231,
                                     stable_iteration_count_threshold=3, max_iteration_count=100):
    """cell_graph_label_propagation over edge arrays in device memory (as dev_cell_graph_edges_to_device left them)."""
    cells = np.ascontiguousarray(vertex_cell_ids, dtype=np.uint32)
    clusters = np.zeros(len(cells), dtype=np.uint32)
    iterations = ctypes.c_uint64(0)
    check(load().em2_dev_cell_graph_label_propagation(_ptr(cells), len(cells), v0_ptr, v1_ptr, sim_ptr, edge_count, seed,
                                                      stable_iteration_count_threshold, max_iteration_count, _ptr(clusters),
                                                      ctypes.byref(iterations)))
    return clusters, int(iterations.value)


def cell_graph_label_propagation(vertex_cell_ids, edge_vertex0, edge_vertex1, edge_similarity, seed=231,
                                 stable_iteration_count_threshold=3, max_iteration_count=100):
    """CellGraph::labelPropagationClustering (src/CellGraph.cpp:443-612) -> (clusterId per vertex, iterations run).
    Host code by nature (a serial schedule defines the result); defaults are ClusterGraphCreationParameters'
    (src/ClusterGraph.hpp:48-50)."""
    cells = np.ascontiguousarray(vertex_cell_ids, dtype=np.uint32)
    v0 = np.ascontiguousarray(edge_vertex0, dtype=np.uint32)
    v1 = np.ascontiguousarray(edge_vertex1, dtype=np.uint32)
    sim = np.ascontiguousarray(edge_similarity, dtype=np.float32)
    if not (len(v0) == len(v1) == len(sim)):
        raise ValueError("the three edge arrays must have one entry per edge")
    clusters = np.zeros(len(cells), dtype=np.uint32)
    iterations = ctypes.c_uint64(0)
    check(load().em2_cell_graph_label_propagation(_ptr(cells), len(cells), _ptr(v0), _ptr(v1), _ptr(sim), len(v0),
                                                  seed, stable_iteration_count_threshold, max_iteration_count,
                                                  _ptr(clusters), ctypes.byref(iterations)))
    return clusters, int(iterations.value)


def cluster_average_expression(toc, data, gene_count, cluster_cells, cluster_offsets):
    """ExpressionMatrix::computeAverageExpression, L2 (src/ExpressionMatrix.cpp:1179-1296), for the clusters
    cluster_cells[cluster_offsets[c]:cluster_offsets[c + 1]] (rows of the CSR, in the order of the additions)
    -> float64 [clusters, genes]."""
    toc = np.ascontiguousarray(toc, dtype=np.uint64)
    data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
    cells = np.ascontiguousarray(cluster_cells, dtype=np.uint32)
    offsets = np.ascontiguousarray(cluster_offsets, dtype=np.uint64)
    clusters = len(offsets) - 1
    if clusters < 0 or (clusters >= 0 and int(offsets[-1]) != len(cells)):
        raise ValueError("cluster_offsets must have one entry per cluster plus one and end at len(cluster_cells)")
    averages = np.zeros((clusters, gene_count), dtype=np.float64)
    check(load().em2_cluster_average_expression(_ptr(toc), _ptr(data), len(toc) - 1, gene_count, _ptr(cells), _ptr(offsets),
                                                clusters, _ptr(averages)))
    return averages


def cluster_similarities(averages, edge_cluster0, edge_cluster1):
    """regressionCoefficient (src/regressionCoefficient.cpp:10-42) of the rows of averages named by every edge -> float64."""
    averages = np.ascontiguousarray(averages, dtype=np.float64)
    e0 = np.ascontiguousarray(edge_cluster0, dtype=np.uint32)
    e1 = np.ascontiguousarray(edge_cluster1, dtype=np.uint32)
    if averages.ndim != 2 or len(e0) != len(e1):
        raise ValueError("averages must be [clusters, genes] and the edge arrays of one length")
    similarity = np.zeros(len(e0), dtype=np.float64)
    check(load().em2_cluster_similarities(_ptr(averages), averages.shape[0], averages.shape[1], _ptr(e0), _ptr(e1), len(e0),
                                          _ptr(similarity)))
    return similarity


def cluster_graph_create(toc, data, gene_count, vertex_rows, edge_vertex0, edge_vertex1, labels, min_cluster_size=100, k=3,
                         similarity_threshold=0.5, similarity_threshold_for_merge=0.9):
    """ExpressionMatrix::createClusterGraph after the label propagation (src/ExpressionMatrix.cpp:2153-2181) -> dict:
    clusterIds (per surviving vertex, in vertex order), cellOffsets / cells and unclusteredCells (cell-graph vertex
    indices), averages [clusters, genes], edgeCluster0 / edgeCluster1 / edgeSimilarity (creation order), facts.
    vertex_rows None: vertex v is row v of the CSR."""
    toc = np.ascontiguousarray(toc, dtype=np.uint64)
    data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
    labels = np.ascontiguousarray(labels, dtype=np.uint32)
    rows = None if vertex_rows is None else np.ascontiguousarray(vertex_rows, dtype=np.uint32)
    v0 = np.ascontiguousarray(edge_vertex0, dtype=np.uint32)
    v1 = np.ascontiguousarray(edge_vertex1, dtype=np.uint32)
    if len(v0) != len(v1) or (rows is not None and len(rows) != len(labels)):
        raise ValueError("one label (and row) per vertex and two vertices per edge are needed")
    lib = load()
    handle = ctypes.c_void_p(None)
    check(lib.em2_cluster_graph_create(_ptr(toc), _ptr(data), len(toc) - 1, gene_count, None if rows is None else _ptr(rows),
                                       len(labels), _ptr(v0), _ptr(v1), len(v0), _ptr(labels), min_cluster_size, k,
                                       similarity_threshold, similarity_threshold_for_merge, ctypes.byref(handle)))
    try:
        clusters, genes = ctypes.c_uint32(0), ctypes.c_uint32(0)
        clustered, unclustered, edges = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        check(lib.em2_cluster_graph_sizes(handle, ctypes.byref(clusters), ctypes.byref(genes), ctypes.byref(clustered),
                                          ctypes.byref(unclustered), ctypes.byref(edges)))
        out = {
            "clusterIds": np.zeros(clusters.value, dtype=np.uint32),
            "cellOffsets": np.zeros(clusters.value + 1, dtype=np.uint64),
            "cells": np.zeros(clustered.value, dtype=np.uint32),
            "unclusteredCells": np.zeros(unclustered.value, dtype=np.uint32),
            "averages": np.zeros((clusters.value, genes.value), dtype=np.float64),
            "edgeCluster0": np.zeros(edges.value, dtype=np.uint32),
            "edgeCluster1": np.zeros(edges.value, dtype=np.uint32),
            "edgeSimilarity": np.zeros(edges.value, dtype=np.float64),
        }
        check(lib.em2_cluster_graph_get(handle, *[_ptr(out[key]) for key in (
            "clusterIds", "cellOffsets", "cells", "unclusteredCells", "averages", "edgeCluster0", "edgeCluster1",
            "edgeSimilarity")]))
        facts = np.zeros(5, dtype=np.float64)
        check(lib.em2_cluster_graph_facts(handle, _ptr(facts), len(facts)))
        out["facts"] = {"seconds": facts[0], "averagesSeconds": facts[1], "similaritiesSeconds": facts[2],
                        "initialClusterCount": int(facts[3]), "initialEdgeCount": int(facts[4])}
    finally:
        lib.em2_cluster_graph_free(handle)
    return out


def signature_graph_take(handle):
    """The content of an em2_signature_graph as a dict, and the handle freed: distinctCount, vertexSignatures uint64 [V, W],
    cellOffsets uint64 [V + 1], cells uint32 (ids local to the cell set), edgeVertex0 / edgeVertex1 uint32 [E]."""
    lib = load()
    try:
        distinct, cells, edges = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        vertices, words = ctypes.c_uint32(0), ctypes.c_uint32(0)
        check(lib.em2_signature_graph_sizes(handle, ctypes.byref(distinct), ctypes.byref(vertices), ctypes.byref(words),
                                            ctypes.byref(cells), ctypes.byref(edges)))
        out = {
            "vertexSignatures": np.zeros((vertices.value, words.value), dtype=np.uint64),
            "cellOffsets": np.zeros(vertices.value + 1, dtype=np.uint64),
            "cells": np.zeros(cells.value, dtype=np.uint32),
            "edgeVertex0": np.zeros(edges.value, dtype=np.uint32),
            "edgeVertex1": np.zeros(edges.value, dtype=np.uint32),
        }
        check(lib.em2_signature_graph_get(handle, *[_ptr(out[key]) for key in (
            "vertexSignatures", "cellOffsets", "cells", "edgeVertex0", "edgeVertex1")]))
        out["distinctCount"] = distinct.value
    finally:
        lib.em2_signature_graph_free(handle)
    return out


def _signatures_2d(signatures, lsh_count):
    signatures = np.ascontiguousarray(signatures, dtype=np.uint64)
    if signatures.ndim != 2 or signatures.shape[1] != word_count(lsh_count):
        raise ValueError("signatures must be [cells, %d] uint64 for %d bits" % (word_count(lsh_count), lsh_count))
    return signatures


def signature_graph_create(signatures, lsh_count, min_cell_count=0):
    """createSignatureGraph after its lookups (em2_signature_graph_create) on host signatures [cells, words] -> the dict
    of signature_graph_take."""
    signatures = _signatures_2d(signatures, lsh_count)
    handle = ctypes.c_void_p(None)
    check(load().em2_signature_graph_create(_ptr(signatures), signatures.shape[0], lsh_count, min_cell_count, ctypes.byref(handle)))
    return signature_graph_take(handle)


def dev_signature_graph_create(signatures, lsh_count, min_cell_count=0):
    """The same through em2_dev_signature_graph_create on a torch device buffer."""
    import torch
    signatures = _signatures_2d(signatures, lsh_count)
    d_signatures = torch.from_numpy(signatures.view(np.int64).copy()).to(torch.device("cuda"))
    torch.cuda.synchronize()
    handle = ctypes.c_void_p(None)
    check(load().em2_dev_signature_graph_create(d_signatures.data_ptr(), signatures.shape[0], lsh_count, min_cell_count,
                                                ctypes.byref(handle)))
    return signature_graph_take(handle)


def lsh_signature_statistics(signatures, lsh_count):
    """The counts of Lsh::writeSignatureStatistics (em2_lsh_signature_statistics): the cells with every bit set, uint64 [lshCount]."""
    signatures = _signatures_2d(signatures, lsh_count)
    set_count = np.zeros(lsh_count, dtype=np.uint64)
    check(load().em2_lsh_signature_statistics(_ptr(signatures), signatures.shape[0], lsh_count, _ptr(set_count)))
    return set_count


def analyze_lsh_signatures(signatures, lsh_count, directory=None):
    """analyzeLshSignatures from its signatures on (em2_analyze_lsh_signatures): writes Signatures.csv, Histogram.csv and
    LshSignatureStatistics.csv into `directory` (None: the working directory)."""
    signatures = _signatures_2d(signatures, lsh_count)
    check(load().em2_analyze_lsh_signatures(_ptr(signatures), signatures.shape[0], lsh_count,
                                            os.fsencode(directory) if directory else None))


GENE_GRAPH_KEYS = ("vertices", "edgeGene0", "edgeGene1", "edgeSimilarity", "connectivityOffsets", "connectivityGenes",
                   "connectivitySimilarities")


def gene_graph_take(handle):
    """The content of an em2_gene_graph as a dict, and the handle freed: vertices uint32 [V] (the genes that stay), edgeGene0 /
    edgeGene1 uint32 [E] and edgeSimilarity float32 [E] in insertion order, connectivityOffsets uint64 [genes + 1],
    connectivityGenes uint32 [2 E] and connectivitySimilarities float32 [2 E] (the neighbours of a gene ascending), removedCount.
    Every id is local to the graph's gene set."""
    lib = load()
    try:
        vertices, removed, edges = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
        check(lib.em2_gene_graph_sizes(handle, ctypes.byref(vertices), ctypes.byref(edges), ctypes.byref(removed)))
        out = {
            "vertices": np.zeros(vertices.value, dtype=np.uint32),
            "edgeGene0": np.zeros(edges.value, dtype=np.uint32),
            "edgeGene1": np.zeros(edges.value, dtype=np.uint32),
            "edgeSimilarity": np.zeros(edges.value, dtype=np.float32),
            "connectivityOffsets": np.zeros(vertices.value + removed.value + 1, dtype=np.uint64),
            "connectivityGenes": np.zeros(2 * edges.value, dtype=np.uint32),
            "connectivitySimilarities": np.zeros(2 * edges.value, dtype=np.float32),
        }
        check(lib.em2_gene_graph_get(handle, *[_ptr(out[key]) for key in GENE_GRAPH_KEYS]))
        out["removedCount"] = removed.value
    finally:
        lib.em2_gene_graph_free(handle)
    return out


def _gene_graph_arguments(pairs, used_count, pairs_gene_set, graph_gene_set):
    pairs = np.ascontiguousarray(pairs, dtype=PAIR_DTYPE)
    used_count = np.ascontiguousarray(used_count, dtype=np.uint32)
    pairs_genes = np.ascontiguousarray(pairs_gene_set, dtype=np.uint32)
    graph_genes = np.ascontiguousarray(graph_gene_set, dtype=np.uint32)
    if pairs.ndim != 2 or pairs.shape[0] != len(pairs_genes) or used_count.shape != (len(pairs_genes),):
        raise ValueError("pairs must be [genes of the pairs' gene set, k] and used_count [genes of the pairs' gene set]")
    return pairs, used_count, pairs_genes, graph_genes


def gene_graph_create(pairs, used_count, pairs_gene_set, graph_gene_set, similarity_threshold, max_connectivity):
    """The GeneGraph constructor and getConnectivity (em2_gene_graph_create) on a host SimilarGenePairs content -> the dict of
    gene_graph_take.  max_connectivity is the reference's int: 0 and negative values mean no limit."""
    pairs, used_count, pairs_genes, graph_genes = _gene_graph_arguments(pairs, used_count, pairs_gene_set, graph_gene_set)
    handle = ctypes.c_void_p(None)
    check(load().em2_gene_graph_create(_ptr(pairs), _ptr(used_count), len(pairs_genes), pairs.shape[1], _ptr(pairs_genes),
                                       _ptr(graph_genes), len(graph_genes), similarity_threshold, int(max_connectivity) % 2 ** 64,
                                       ctypes.byref(handle)))
    return gene_graph_take(handle)


def dev_gene_graph_create(pairs, used_count, pairs_gene_set, graph_gene_set, similarity_threshold, max_connectivity):
    """The same through em2_dev_gene_graph_create: pairs and used_count go to torch device buffers first."""
    import torch
    pairs, used_count, pairs_genes, graph_genes = _gene_graph_arguments(pairs, used_count, pairs_gene_set, graph_gene_set)
    device = torch.device("cuda")
    d_pairs = torch.from_numpy(pairs.view(np.int64).reshape(-1).copy()).to(device)
    d_used = torch.from_numpy(used_count.view(np.int32).copy()).to(device)
    torch.cuda.synchronize()
    handle = ctypes.c_void_p(None)
    check(load().em2_dev_gene_graph_create(d_pairs.data_ptr() if d_pairs.numel() else None, d_used.data_ptr() if d_used.numel() else None,
                                           len(pairs_genes), pairs.shape[1], _ptr(pairs_genes), _ptr(graph_genes), len(graph_genes),
                                           similarity_threshold, int(max_connectivity) % 2 ** 64, ctypes.byref(handle)))
    return gene_graph_take(handle)


class LayoutParameters(_c.Structure):
    """em2_layout_parameters, with the defaults of include/em2_lsh.h."""
    _fields_ = [("seed", _c.c_uint32), ("maxIterationCount", _c.c_uint32), ("tolerance", _c.c_double), ("gravity", _c.c_double),
                ("initialStep", _c.c_double)]

    def __init__(self, seed=231, maxIterationCount=300, tolerance=0.01, gravity=0.02, initialStep=1.0):
        super().__init__(seed, maxIterationCount, tolerance, gravity, initialStep)


class LayoutResult(_c.Structure):
    """em2_layout_result."""
    _fields_ = [("iterationCount", _c.c_uint32), ("reserved", _c.c_uint32), ("step", _c.c_double), ("energy", _c.c_double)]


def _layout_edges(vertex_count, edge_vertex0, edge_vertex1):
    v0 = np.ascontiguousarray(edge_vertex0, dtype=np.uint32)
    v1 = np.ascontiguousarray(edge_vertex1, dtype=np.uint32)
    if v0.ndim != 1 or v0.shape != v1.shape:
        raise ValueError("edge_vertex0 and edge_vertex1 must be one-dimensional and of one length")
    return int(vertex_count), v0, v1


LAYOUT_DEPTH_AUTO = 0xffffffff                                # EM2_LAYOUT_DEPTH_AUTO
LAYOUT_MAX_DEPTH = 10                                         # EM2_LAYOUT_MAX_DEPTH
LAYOUT_LEAF_TARGET = 8                                        # EM2_LAYOUT_LEAF_TARGET


def _depth(depth):
    """The depth argument of a pyramid entry as a tuple to splice into the call; none for an exact entry (depth None)."""
    return () if depth is None else (int(depth) % 2 ** 32,)


def graph_layout(vertex_count, edge_vertex0, edge_vertex1, parameters=None, _depth_argument=None):
    """em2_graph_layout -> (x float32 [V], y float32 [V], iterations, final step, final energy).  parameters: a
    LayoutParameters (None: the defaults)."""
    n, v0, v1 = _layout_edges(vertex_count, edge_vertex0, edge_vertex1)
    parameters = parameters if parameters is not None else LayoutParameters()
    x, y = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    result = LayoutResult()
    entry = load().em2_graph_layout if _depth_argument is None else load().em2_graph_layout_pyramid
    check(entry(n, _ptr(v0), _ptr(v1), len(v0), ctypes.byref(parameters), *_depth(_depth_argument), _ptr(x), _ptr(y), ctypes.byref(result)))
    return x, y, result.iterationCount, result.step, result.energy


def graph_layout_pyramid(vertex_count, edge_vertex0, edge_vertex1, parameters=None, depth=LAYOUT_DEPTH_AUTO):
    """em2_graph_layout_pyramid: the same with the repulsion approximated beyond a vertex's neighbourhood.
    depth: LAYOUT_DEPTH_AUTO or 0 ... LAYOUT_MAX_DEPTH."""
    return graph_layout(vertex_count, edge_vertex0, edge_vertex1, parameters, _depth_argument=depth)


def dev_graph_layout_pyramid(vertex_count, edge_vertex0, edge_vertex1, parameters=None, depth=LAYOUT_DEPTH_AUTO):
    """The same through em2_dev_graph_layout_pyramid."""
    return dev_graph_layout(vertex_count, edge_vertex0, edge_vertex1, parameters, _depth_argument=depth)


def dev_graph_layout(vertex_count, edge_vertex0, edge_vertex1, parameters=None, _depth_argument=None):
    """The same through em2_dev_graph_layout: the edges go to torch device buffers first, the positions come back from two."""
    import torch
    n, v0, v1 = _layout_edges(vertex_count, edge_vertex0, edge_vertex1)
    parameters = parameters if parameters is not None else LayoutParameters()
    device = torch.device("cuda")
    d_v0 = torch.from_numpy(v0.view(np.int32).copy()).to(device)
    d_v1 = torch.from_numpy(v1.view(np.int32).copy()).to(device)
    d_x = torch.zeros(n, dtype=torch.float32, device=device)
    d_y = torch.zeros(n, dtype=torch.float32, device=device)
    torch.cuda.synchronize()
    result = LayoutResult()
    entry = load().em2_dev_graph_layout if _depth_argument is None else load().em2_dev_graph_layout_pyramid
    check(entry(n, d_v0.data_ptr() if len(v0) else None, d_v1.data_ptr() if len(v0) else None, len(v0), ctypes.byref(parameters),
                *_depth(_depth_argument), d_x.data_ptr() if n else None, d_y.data_ptr() if n else None, ctypes.byref(result)))
    return d_x.cpu().numpy(), d_y.cpu().numpy(), result.iterationCount, result.step, result.energy


def graph_layout_forces_pyramid(vertex_count, edge_vertex0, edge_vertex1, gravity, x, y, depth=LAYOUT_DEPTH_AUTO):
    """em2_graph_layout_forces_pyramid (for tests): the same evaluation with the approximated repulsion."""
    return graph_layout_forces(vertex_count, edge_vertex0, edge_vertex1, gravity, x, y, _depth_argument=depth)


def graph_layout_forces(vertex_count, edge_vertex0, edge_vertex1, gravity, x, y, _depth_argument=None):
    """em2_graph_layout_forces (for tests): one evaluation at the positions x / y -> (fx float32 [V], fy float32 [V], energy)."""
    n, v0, v1 = _layout_edges(vertex_count, edge_vertex0, edge_vertex1)
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    if x.shape != (n,) or y.shape != (n,):
        raise ValueError("x and y must hold one position per vertex")
    fx, fy = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    energy = ctypes.c_double(0.)
    entry = load().em2_graph_layout_forces if _depth_argument is None else load().em2_graph_layout_forces_pyramid
    check(entry(n, _ptr(v0), _ptr(v1), len(v0), float(gravity), *_depth(_depth_argument), _ptr(x), _ptr(y), _ptr(fx), _ptr(fy),
                ctypes.byref(energy)))
    return fx, fy, energy.value


LAYOUT_DEPTH_EXACT = 0xfffffffe                               # EM2_LAYOUT_DEPTH_EXACT
LAYOUT_COARSEST = 32                                          # EM2_LAYOUT_COARSEST
LAYOUT_MAX_LEVELS = 32                                        # EM2_LAYOUT_MAX_LEVELS
LAYOUT_EXACT_LIMIT = 4096                                     # EM2_LAYOUT_EXACT_LIMIT


class LayoutLevels(_c.Structure):
    """em2_layout_levels."""
    _fields_ = [("levelCount", _c.c_uint32), ("reserved", _c.c_uint32), ("vertexCount", _c.c_uint32 * LAYOUT_MAX_LEVELS),
                ("matchingRounds", _c.c_uint32 * LAYOUT_MAX_LEVELS), ("iterationCount", _c.c_uint32 * LAYOUT_MAX_LEVELS),
                ("reserved2", _c.c_uint32 * LAYOUT_MAX_LEVELS), ("edgeCount", _c.c_uint64 * LAYOUT_MAX_LEVELS)]

    def as_list(self):
        """[(vertexCount, edgeCount, matchingRounds, iterationCount)], level 0 first."""
        return [(self.vertexCount[l], self.edgeCount[l], self.matchingRounds[l], self.iterationCount[l]) for l in range(self.levelCount)]


def graph_layout_multilevel(vertex_count, edge_vertex0, edge_vertex1, parameters=None, depth=LAYOUT_DEPTH_EXACT):
    """em2_graph_layout_multilevel -> (x float32 [V], y float32 [V], iterations of all levels, final step, final
    energy, levels: [(vertexCount, edgeCount, matchingRounds, iterationCount)], level 0 first).  depth: LAYOUT_DEPTH_EXACT,
    LAYOUT_DEPTH_AUTO or 0 ... LAYOUT_MAX_DEPTH."""
    n, v0, v1 = _layout_edges(vertex_count, edge_vertex0, edge_vertex1)
    parameters = parameters if parameters is not None else LayoutParameters()
    x, y = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    result, levels = LayoutResult(), LayoutLevels()
    check(load().em2_graph_layout_multilevel(n, _ptr(v0), _ptr(v1), len(v0), ctypes.byref(parameters), int(depth) % 2 ** 32, _ptr(x), _ptr(y),
                                             ctypes.byref(result), ctypes.byref(levels)))
    return x, y, result.iterationCount, result.step, result.energy, levels.as_list()


def dev_graph_layout_multilevel(vertex_count, edge_vertex0, edge_vertex1, parameters=None, depth=LAYOUT_DEPTH_EXACT):
    """The same through em2_dev_graph_layout_multilevel."""
    import torch
    n, v0, v1 = _layout_edges(vertex_count, edge_vertex0, edge_vertex1)
    parameters = parameters if parameters is not None else LayoutParameters()
    device = torch.device("cuda")
    d_v0 = torch.from_numpy(v0.view(np.int32).copy()).to(device)
    d_v1 = torch.from_numpy(v1.view(np.int32).copy()).to(device)
    d_x = torch.zeros(n, dtype=torch.float32, device=device)
    d_y = torch.zeros(n, dtype=torch.float32, device=device)
    torch.cuda.synchronize()
    result, levels = LayoutResult(), LayoutLevels()
    check(load().em2_dev_graph_layout_multilevel(n, d_v0.data_ptr() if len(v0) else None, d_v1.data_ptr() if len(v0) else None, len(v0),
                                                 ctypes.byref(parameters), int(depth) % 2 ** 32, d_x.data_ptr() if n else None,
                                                 d_y.data_ptr() if n else None, ctypes.byref(result), ctypes.byref(levels)))
    return d_x.cpu().numpy(), d_y.cpu().numpy(), result.iterationCount, result.step, result.energy, levels.as_list()


def _optional_u32(a, count, what):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.uint32)
    if a.shape != (count,):
        raise ValueError("%s must hold %d values" % (what, count))
    return a


def graph_layout_coarsen(vertex_count, edge_vertex0, edge_vertex1, seed, level, mass=None, edge_weight=None):
    """em2_graph_layout_coarsen (for tests): one coarsening step -> dict: mate, coarseOf uint32 [V], coarseCount, rounds,
    coarseMass uint32 [coarseCount], coarseEdges (a, b, w), each uint32 and ascending by (a, b)."""
    n, v0, v1 = _layout_edges(vertex_count, edge_vertex0, edge_vertex1)
    mass, edge_weight = _optional_u32(mass, n, "mass"), _optional_u32(edge_weight, len(v0), "edge_weight")
    mate, coarse_of, coarse_mass = (np.zeros(n, dtype=np.uint32) for _ in range(3))
    a, b, w = (np.zeros(len(v0), dtype=np.uint32) for _ in range(3))
    count, rounds, edge_count = _c.c_uint32(0), _c.c_uint32(0), _c.c_uint64(0)
    check(load().em2_graph_layout_coarsen(n, None if mass is None else _ptr(mass), _ptr(v0), _ptr(v1),
                                          None if edge_weight is None else _ptr(edge_weight), len(v0), int(seed), int(level), _ptr(mate),
                                          _ptr(coarse_of), ctypes.byref(count), ctypes.byref(rounds), _ptr(coarse_mass), _ptr(a), _ptr(b),
                                          _ptr(w), ctypes.byref(edge_count)))
    m = edge_count.value
    return dict(mate=mate, coarseOf=coarse_of, coarseCount=count.value, rounds=rounds.value, coarseMass=coarse_mass[:count.value].copy(),
                coarseEdges=(a[:m].copy(), b[:m].copy(), w[:m].copy()))


def graph_layout_forces_weighted(vertex_count, edge_vertex0, edge_vertex1, gravity, x, y, depth=LAYOUT_DEPTH_EXACT, mass=None,
                                 edge_weight=None):
    """em2_graph_layout_forces_weighted (for tests): one evaluation with masses and edge weights -> (fx, fy, energy)."""
    n, v0, v1 = _layout_edges(vertex_count, edge_vertex0, edge_vertex1)
    mass, edge_weight = _optional_u32(mass, n, "mass"), _optional_u32(edge_weight, len(v0), "edge_weight")
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    if x.shape != (n,) or y.shape != (n,):
        raise ValueError("x and y must hold one position per vertex")
    fx, fy = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    energy = ctypes.c_double(0.)
    check(load().em2_graph_layout_forces_weighted(n, None if mass is None else _ptr(mass), _ptr(v0), _ptr(v1),
                                                  None if edge_weight is None else _ptr(edge_weight), len(v0), float(gravity),
                                                  int(depth) % 2 ** 32, _ptr(x), _ptr(y), _ptr(fx), _ptr(fy), ctypes.byref(energy)))
    return fx, fy, energy.value


CONTINGENCY_AUTOMATIC, CONTINGENCY_LDS, CONTINGENCY_SORT = 0, 1, 2
CONTINGENCY_LDS_CELLS = 16384


def contingency_take(handle):
    """The content of an em2_contingency as a dict, and the handle freed: rowTotals uint64 [n0], columnTotals uint64 [n1], the
    cells that are not zero as i0 / i1 uint32 and count uint64, ascending by (i0, i1), the three sums as Python ints (sumCells,
    sumRows, sumColumns), n, and path: the one that ran (CONTINGENCY_LDS or CONTINGENCY_SORT)."""
    lib = load()
    try:
        n0, n1, path = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_int(0)
        n, nonzero = ctypes.c_uint64(0), ctypes.c_uint64(0)
        check(lib.em2_contingency_sizes(handle, ctypes.byref(n0), ctypes.byref(n1), ctypes.byref(n), ctypes.byref(nonzero),
                                        ctypes.byref(path)))
        out = {
            "rowTotals": np.zeros(n0.value, dtype=np.uint64),
            "columnTotals": np.zeros(n1.value, dtype=np.uint64),
            "i0": np.zeros(nonzero.value, dtype=np.uint32),
            "i1": np.zeros(nonzero.value, dtype=np.uint32),
            "count": np.zeros(nonzero.value, dtype=np.uint64),
        }
        sums = np.zeros(3, dtype=np.uint64)
        check(lib.em2_contingency_get(handle, *[_ptr(out[key]) for key in ("rowTotals", "columnTotals", "i0", "i1", "count")],
                                      _ptr(sums)))
        out["sumCells"], out["sumRows"], out["sumColumns"] = (int(x) for x in sums)
        out["n"] = int(n.value)
        out["path"] = path.value
    finally:
        lib.em2_contingency_free(handle)
    return out


def _contingency_ids(id0, id1):
    id0 = np.ascontiguousarray(id0, dtype=np.uint32)
    id1 = np.ascontiguousarray(id1, dtype=np.uint32)
    if id0.ndim != 1 or id0.shape != id1.shape:
        raise ValueError("id0 and id1 must be one-dimensional and equally long")
    return id0, id1


def contingency(id0, id1, n0, n1, path=CONTINGENCY_AUTOMATIC):
    """The contingency table of two labelings (em2_contingency_create) -> the dict of contingency_take."""
    id0, id1 = _contingency_ids(id0, id1)
    handle = ctypes.c_void_p(None)
    check(load().em2_contingency_create(_ptr(id0), _ptr(id1), len(id0), n0, n1, path, ctypes.byref(handle)))
    return contingency_take(handle)


def dev_contingency(d_id0_ptr, d_id1_ptr, n, n0, n1, path=CONTINGENCY_AUTOMATIC):
    """The same on ids that are in device memory already (em2_dev_contingency): two device pointers to n uint32 each."""
    handle = ctypes.c_void_p(None)
    check(load().em2_dev_contingency(d_id0_ptr, d_id1_ptr, n, n0, n1, path, ctypes.byref(handle)))
    return contingency_take(handle)


def rand_index(sum_cells, sum_rows, sum_columns, n):
    """computeRandIndex (src/randIndex.hpp:58-97) from the three sums of a contingency table -> (randIndex, adjustedRandIndex)."""
    ri, ari = ctypes.c_double(0.), ctypes.c_double(0.)
    check(load().em2_rand_index(sum_cells, sum_rows, sum_columns, n, ctypes.byref(ri), ctypes.byref(ari)))
    return ri.value, ari.value


GRAPH_COMPARE_TABLE, GRAPH_COMPARE_LIST = 0, 1


def graph_comparison_take(handle):
    """The content of an em2_graph_comparison as a dict, and the handle freed: commonVertexCount, edgeCount0, edgeCount1 (distinct
    unordered cell pairs), commonEdgeCount, commonIdenticalEdgeCount as Python ints, binDelta float32 and binCount uint64
    ascending by binDelta, and path: the one that ran."""
    lib = load()
    try:
        words = [ctypes.c_uint64(0) for _ in range(6)]
        path = ctypes.c_int(0)
        check(lib.em2_graph_comparison_sizes(handle, *[ctypes.byref(w) for w in words], ctypes.byref(path)))
        names = ("commonVertexCount", "edgeCount0", "edgeCount1", "commonEdgeCount", "commonIdenticalEdgeCount")
        out = {name: int(w.value) for name, w in zip(names, words)}
        out["binDelta"] = np.zeros(words[5].value, dtype=np.float32)
        out["binCount"] = np.zeros(words[5].value, dtype=np.uint64)
        check(lib.em2_graph_comparison_get(handle, _ptr(out["binDelta"]), _ptr(out["binCount"])))
        out["path"] = path.value
    finally:
        lib.em2_graph_comparison_free(handle)
    return out


def _compare_graph(graph):
    """(vertexCellIds, edgeVertex0, edgeVertex1, edgeSimilarity) as contiguous arrays of the entry's types."""
    cells, v0, v1, similarity = graph
    cells = np.ascontiguousarray(cells, dtype=np.uint32)
    v0 = np.ascontiguousarray(v0, dtype=np.uint32)
    v1 = np.ascontiguousarray(v1, dtype=np.uint32)
    similarity = np.ascontiguousarray(similarity, dtype=np.float32)
    if cells.ndim != 1 or v0.ndim != 1 or not (v0.shape == v1.shape == similarity.shape):
        raise ValueError("a graph is (vertexCellIds, edgeVertex0, edgeVertex1, edgeSimilarity), the three edge arrays with one "
                         "entry per edge")
    return cells, v0, v1, similarity


def cell_graph_compare(graph0, graph1, path=GRAPH_COMPARE_TABLE):
    """compareCellGraphs (src/ExpressionMatrixHttpServerGraphs.cpp:104-345) without its page, on the GPU (em2_cell_graph_compare):
    each graph is (vertexCellIds, edgeVertex0, edgeVertex1, edgeSimilarity), the edges as vertex indices -> the dict of
    graph_comparison_take."""
    g0, g1 = _compare_graph(graph0), _compare_graph(graph1)
    handle = ctypes.c_void_p(None)
    check(load().em2_cell_graph_compare(_ptr(g0[0]), len(g0[0]), _ptr(g0[1]), _ptr(g0[2]), _ptr(g0[3]), len(g0[1]),
                                        _ptr(g1[0]), len(g1[0]), _ptr(g1[1]), _ptr(g1[2]), _ptr(g1[3]), len(g1[1]),
                                        int(path), ctypes.byref(handle)))
    return graph_comparison_take(handle)


def dev_cell_graph_compare(vertex_cell_ids0, v0_ptr0, v1_ptr0, sim_ptr0, edge_count0, vertex_cell_ids1, v0_ptr1, v1_ptr1, sim_ptr1,
                           edge_count1, path=GRAPH_COMPARE_TABLE):
    """The same over edge arrays in device memory (pointers, as dev_cell_graph_edges_to_device left them); the vertex lists
    are host arrays."""
    cells0 = np.ascontiguousarray(vertex_cell_ids0, dtype=np.uint32)
    cells1 = np.ascontiguousarray(vertex_cell_ids1, dtype=np.uint32)
    handle = ctypes.c_void_p(None)
    check(load().em2_dev_cell_graph_compare(_ptr(cells0), len(cells0), v0_ptr0, v1_ptr0, sim_ptr0, int(edge_count0),
                                            _ptr(cells1), len(cells1), v0_ptr1, v1_ptr1, sim_ptr1, int(edge_count1),
                                            int(path), ctypes.byref(handle)))
    return graph_comparison_take(handle)


def group_colors_take(handle):
    """The content of an em2_group_colors as a dict, and the handle freed: groupCount, pairGroup0 < pairGroup1 uint32 ascending
    with pairEdgeCount uint64 (the group graph), colorTable uint32 [groupCount], and path: the contingency path that ran (0
    where there was no edge)."""
    lib = load()
    try:
        groups, pairs, path = ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_int(0)
        check(lib.em2_group_colors_sizes(handle, ctypes.byref(groups), ctypes.byref(pairs), ctypes.byref(path)))
        out = {
            "groupCount": int(groups.value),
            "pairGroup0": np.zeros(pairs.value, dtype=np.uint32),
            "pairGroup1": np.zeros(pairs.value, dtype=np.uint32),
            "pairEdgeCount": np.zeros(pairs.value, dtype=np.uint64),
            "colorTable": np.zeros(groups.value, dtype=np.uint32),
            "path": path.value,
        }
        check(lib.em2_group_colors_get(handle, *[_ptr(out[key]) for key in ("pairGroup0", "pairGroup1", "pairEdgeCount", "colorTable")]))
    finally:
        lib.em2_group_colors_free(handle)
    return out


def graph_group_colors(vertex_group, edge_vertex0, edge_vertex1, path=CONTINGENCY_AUTOMATIC):
    """CellGraph::assignColorsToGroups (src/CellGraph.cpp:794-862): the group graph of the edges (on the GPU, through the
    contingency code) and the reference's greedy colouring of it (em2_graph_group_colors) -> the dict of group_colors_take."""
    group = np.ascontiguousarray(vertex_group, dtype=np.uint32)
    v0 = np.ascontiguousarray(edge_vertex0, dtype=np.uint32)
    v1 = np.ascontiguousarray(edge_vertex1, dtype=np.uint32)
    if group.ndim != 1 or v0.ndim != 1 or v0.shape != v1.shape:
        raise ValueError("one group per vertex and two vertices per edge are needed")
    handle = ctypes.c_void_p(None)
    check(load().em2_graph_group_colors(_ptr(group), len(group), _ptr(v0), _ptr(v1), len(v0), int(path), ctypes.byref(handle)))
    return group_colors_take(handle)


def dev_graph_group_colors(vertex_group, v0_ptr, v1_ptr, edge_count, path=CONTINGENCY_AUTOMATIC):
    """The same over edge arrays in device memory (pointers); the groups are a host array."""
    group = np.ascontiguousarray(vertex_group, dtype=np.uint32)
    handle = ctypes.c_void_p(None)
    check(load().em2_dev_graph_group_colors(_ptr(group), len(group), v0_ptr, v1_ptr, int(edge_count), int(path), ctypes.byref(handle)))
    return group_colors_take(handle)


def meta_data_table_take(handle, cell_rows=False):
    """The content of an em2_meta_data_table as a dict, and the handle freed: values0 / values1 (lists of str) with counts0 /
    counts1 (lists of int) in histogram order, triples [(row, column, count)], sums (four ints: the three of the contingency
    table and n), path; with cell_rows also cellRow (uint32, per cell of the set the place of its value in values0)."""
    lib = load()
    try:
        sizes = [ctypes.c_uint64(0) for _ in range(5)]
        path = ctypes.c_int(0)
        check(lib.em2_meta_data_table_sizes(handle, *[ctypes.byref(s) for s in sizes], ctypes.byref(path)))
        count0, count1, bytes0, bytes1, nonzero = (int(s.value) for s in sizes)
        values = [ctypes.create_string_buffer(max(bytes0, 1)), ctypes.create_string_buffer(max(bytes1, 1))]
        counts = [np.zeros(count0, dtype=np.uint64), np.zeros(count1, dtype=np.uint64)]
        triples = [np.zeros(nonzero, dtype=np.uint64) for _ in range(3)]
        sums = np.zeros(4, dtype=np.uint64)
        check(lib.em2_meta_data_table_get(handle, values[0], _ptr(counts[0]), values[1], _ptr(counts[1]), _ptr(triples[0]),
                                          _ptr(triples[1]), _ptr(triples[2]), _ptr(sums)))
        out = {"path": path.value, "sums": [int(x) for x in sums],
               "triples": list(zip(*(t.tolist() for t in triples)))}
        for f, size in enumerate((bytes0, bytes1)):
            out["values%d" % f] = [v.decode("utf-8", "surrogateescape") for v in values[f].raw[:size].split(b"\0")[:-1]]
            out["counts%d" % f] = counts[f].tolist()
        if cell_rows:
            out["cellRow"] = np.zeros(out["sums"][3], dtype=np.uint32)
            if len(out["cellRow"]):
                check(lib.em2_meta_data_table_cell_rows(handle, _ptr(out["cellRow"])))
    finally:
        lib.em2_meta_data_table_free(handle)
    return out


def analyze_lsh(toc, data, gene_count, signatures, lsh_count, global_cell_ids, seed, csv_downsample, pairs_csv_path,
                statistics_csv_path=None, per_pair=False):
    """ExpressionMatrix::analyzeLsh on a subset's counts and signatures (em2_analyze_lsh) -> dict(sum0, sum1, sum2[, exact,
    lsh]); writes the two csv files."""
    toc = np.ascontiguousarray(toc, dtype=np.uint64)
    data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
    signatures = np.ascontiguousarray(signatures, dtype=np.uint64)
    ids = np.ascontiguousarray(global_cell_ids, dtype=np.uint32)
    n = len(toc) - 1
    out = {"sum0": np.zeros(200, dtype=np.uint64), "sum1": np.zeros(200, dtype=np.float64), "sum2": np.zeros(200, dtype=np.float64)}
    pairs = n * (n - 1) // 2
    if per_pair:
        out["exact"] = np.zeros(pairs, dtype=np.float64)
        out["lsh"] = np.zeros(pairs, dtype=np.float64)
    check(load().em2_analyze_lsh(_ptr(toc), _ptr(data), n, gene_count, _ptr(signatures), lsh_count, _ptr(ids), seed,
                                 csv_downsample, os.fsencode(pairs_csv_path),
                                 os.fsencode(statistics_csv_path) if statistics_csv_path else None,
                                 _ptr(out["sum0"]), _ptr(out["sum1"]), _ptr(out["sum2"]),
                                 _ptr(out["exact"]) if per_pair else None, _ptr(out["lsh"]) if per_pair else None))
    return out


def find_similar_pairs0(toc, data, gene_count, k=100, similarity_threshold=0.2):
    """findSimilarPairs0 (exact, all pairs) on a subset's host CSR -> (pairs [cells, k], usedCount, lowestSimilarityIndex,
    lowestSimilarity): the -Pairs content and the three CellInfo fields as SimilarPairs::add and sort leave them."""
    toc = np.ascontiguousarray(toc, dtype=np.uint64)
    data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
    cell_count = len(toc) - 1
    pairs = np.zeros((cell_count, k), dtype=PAIR_DTYPE)
    used = np.zeros(cell_count, dtype=np.uint32)
    lowest_index = np.zeros(cell_count, dtype=np.uint32)
    lowest = np.zeros(cell_count, dtype=np.float32)
    check(load().em2_find_similar_pairs0(_ptr(toc), _ptr(data), cell_count, gene_count, k, similarity_threshold, _ptr(pairs),
                                         _ptr(used), _ptr(lowest_index), _ptr(lowest)))
    return pairs, used, lowest_index, lowest


GENE_PAIRS_BUFFER_MB_DEFAULT = 4096


def cell_norm_inverses(toc, data, gene_count):
    """Cell::norm1Inverse / norm2Inverse of ExpressionMatrix::addCell (src/ExpressionMatrix.cpp:241-263) for the cells of a
    host CSR -> (norm1Inverse, norm2Inverse), float64 [cells].  Host code."""
    toc = np.ascontiguousarray(toc, dtype=np.uint64)
    data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
    cell_count = len(toc) - 1
    norm1 = np.zeros(cell_count, dtype=np.float64)
    norm2 = np.zeros(cell_count, dtype=np.float64)
    check(load().em2_cell_norm_inverses(_ptr(toc), _ptr(data), cell_count, gene_count, _ptr(norm1), _ptr(norm2)))
    return norm1, norm2


def gene_information_content(toc, data, gene_count, norm_inverse=None):
    """computeGeneInformationContent (src/ExpressionMatrix.cpp:1947-2018) for every gene of a subset's host CSR ->
    (informationContent float32 [genes], the same as float64, expressingCellCount uint32 [genes]).  norm_inverse: None (no
    normalisation) or float64 [cells], the cells' norm1Inverse or norm2Inverse."""
    toc = np.ascontiguousarray(toc, dtype=np.uint64)
    data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
    cell_count = len(toc) - 1
    if norm_inverse is not None:
        norm_inverse = np.ascontiguousarray(norm_inverse, dtype=np.float64)
        if len(norm_inverse) != cell_count:
            raise ValueError("norm_inverse must have one value per cell")
    single = np.zeros(gene_count, dtype=np.float32)
    double = np.zeros(gene_count, dtype=np.float64)
    expressing = np.zeros(gene_count, dtype=np.uint32)
    check(load().em2_gene_information_content(_ptr(toc), _ptr(data), cell_count, gene_count,
                                              _ptr(norm_inverse) if norm_inverse is not None else None, _ptr(single),
                                              _ptr(double), _ptr(expressing)))
    return single, double, expressing


def dev_gene_information_content(toc, data, gene_count, norm_inverse=None):
    """The same through em2_dev_gene_information_content on torch device buffers (a stream of torch's)."""
    import torch
    toc = np.ascontiguousarray(toc, dtype=np.uint64)
    data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
    cell_count, entries = len(toc) - 1, len(data)
    lib = load()
    device = torch.device("cuda")
    d_toc = torch.from_numpy(toc.view(np.int64).copy()).to(device)
    d_data = torch.from_numpy(data.view(np.uint8).reshape(-1).copy()).to(device)
    d_norm = torch.from_numpy(np.ascontiguousarray(norm_inverse, dtype=np.float64)).to(device) if norm_inverse is not None else None
    d_single = torch.zeros(gene_count, dtype=torch.float32, device=device)
    d_double = torch.zeros(gene_count, dtype=torch.float64, device=device)
    d_expressing = torch.zeros(gene_count, dtype=torch.int32, device=device)
    workspace_bytes = lib.em2_dev_gene_information_content_workspace(cell_count, gene_count, entries)
    d_workspace = torch.empty(workspace_bytes, dtype=torch.uint8, device=device)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    check(lib.em2_dev_gene_information_content(d_toc.data_ptr(), d_data.data_ptr(), cell_count, gene_count, entries,
                                               d_norm.data_ptr() if d_norm is not None else None, d_single.data_ptr(),
                                               d_double.data_ptr(), d_expressing.data_ptr(), d_workspace.data_ptr(),
                                               workspace_bytes, stream.cuda_stream))
    torch.cuda.current_stream().wait_stream(stream)
    return d_single.cpu().numpy(), d_double.cpu().numpy(), d_expressing.cpu().numpy().view(np.uint32)


NO_GROUP, GROUP_EXCLUDED = 0xffffffff, 0xfffffffe          # EM2_NO_GROUP, EM2_GROUP_EXCLUDED


def rank_genes_arrays(gene_count, group_count):
    """The zeroed outputs of the rank genes entries: groupSize [groups], nonZeroCount and rankSum2 [genes][groups], tieSum
    [genes], zScore and auc [genes][groups]."""
    return {"groupSize": np.zeros(group_count, dtype=np.uint32), "nonZeroCount": np.zeros((gene_count, group_count), dtype=np.uint32),
            "rankSum2": np.zeros((gene_count, group_count), dtype=np.uint64), "tieSum": np.zeros(gene_count, dtype=np.uint64),
            "zScore": np.zeros((gene_count, group_count), dtype=np.float64), "auc": np.zeros((gene_count, group_count), dtype=np.float64)}


def rank_genes(toc, data, gene_count, group, group_count, norm_inverse=None):
    """em2_rank_genes: the rank-sum test of every gene of a subset's host CSR for every group of cells against the rest -> the
    dict of rank_genes_arrays.  group: uint32 [cells], a group below group_count or NO_GROUP."""
    toc = np.ascontiguousarray(toc, dtype=np.uint64)
    data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
    group = np.ascontiguousarray(group, dtype=np.uint32)
    cell_count = len(toc) - 1
    if len(group) != cell_count:
        raise ValueError("group must have one value per cell")
    if norm_inverse is not None:
        norm_inverse = np.ascontiguousarray(norm_inverse, dtype=np.float64)
        if len(norm_inverse) != cell_count:
            raise ValueError("norm_inverse must have one value per cell")
    out = rank_genes_arrays(gene_count, group_count)
    check(load().em2_rank_genes(_ptr(toc), _ptr(data), cell_count, gene_count, _ptr(norm_inverse) if norm_inverse is not None else None,
                                _ptr(group), group_count, _ptr(out["groupSize"]), _ptr(out["nonZeroCount"]), _ptr(out["rankSum2"]),
                                _ptr(out["tieSum"]), _ptr(out["zScore"]), _ptr(out["auc"])))
    return out


def dev_rank_genes(toc, data, gene_count, group, group_count, norm_inverse=None, fill=0):
    """The integers of rank_genes through em2_dev_rank_genes on torch device buffers (a stream of torch's).  The outputs start
    as `fill` in every byte, so that a caller sees what a failed call left of them: on an error the RuntimeError carries them
    as its `outputs`."""
    import torch
    toc = np.ascontiguousarray(toc, dtype=np.uint64)
    data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
    cell_count, entries = len(toc) - 1, len(data)
    lib = load()
    device = torch.device("cuda")
    d_toc = torch.from_numpy(toc.view(np.int64).copy()).to(device)
    d_data = torch.from_numpy(data.view(np.uint8).reshape(-1).copy()).to(device)
    d_group = torch.from_numpy(np.ascontiguousarray(group, dtype=np.uint32).view(np.int32).copy()).to(device)
    d_norm = torch.from_numpy(np.ascontiguousarray(norm_inverse, dtype=np.float64)).to(device) if norm_inverse is not None else None
    counters = gene_count * group_count
    d_out = {"groupSize": torch.full((group_count * 4,), fill, dtype=torch.uint8, device=device),
             "nonZeroCount": torch.full((counters * 4,), fill, dtype=torch.uint8, device=device),
             "rankSum2": torch.full((counters * 8,), fill, dtype=torch.uint8, device=device),
             "tieSum": torch.full((gene_count * 8,), fill, dtype=torch.uint8, device=device)}
    workspace_bytes = lib.em2_dev_rank_genes_workspace(cell_count, gene_count, entries, group_count)
    d_workspace = torch.empty(max(workspace_bytes, 1), dtype=torch.uint8, device=device)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    rc = lib.em2_dev_rank_genes(d_toc.data_ptr(), d_data.data_ptr(), cell_count, gene_count, entries,
                                d_norm.data_ptr() if d_norm is not None else None, d_group.data_ptr(), group_count,
                                d_out["groupSize"].data_ptr(), d_out["nonZeroCount"].data_ptr(), d_out["rankSum2"].data_ptr(),
                                d_out["tieSum"].data_ptr(), d_workspace.data_ptr(), workspace_bytes, stream.cuda_stream)
    torch.cuda.current_stream().wait_stream(stream)
    out = {"groupSize": d_out["groupSize"].cpu().numpy().view(np.uint32),
           "nonZeroCount": d_out["nonZeroCount"].cpu().numpy().view(np.uint32).reshape(gene_count, group_count),
           "rankSum2": d_out["rankSum2"].cpu().numpy().view(np.uint64).reshape(gene_count, group_count),
           "tieSum": d_out["tieSum"].cpu().numpy().view(np.uint64)}
    try:
        check(rc)
    except RuntimeError as error:
        error.outputs = out
        raise
    return out


DENSE_FLOAT64, DENSE_FLOAT32 = 0, 1
DENSE_ELEMENT_TYPES = {np.dtype(np.float64): DENSE_FLOAT64, np.dtype(np.float32): DENSE_FLOAT32}


def dense_element_type(dtype):
    """EM2_DENSE_FLOAT64 / EM2_DENSE_FLOAT32 for np.float64 / np.float32; ValueError for anything else."""
    try:
        return DENSE_ELEMENT_TYPES[np.dtype(dtype)]
    except (KeyError, TypeError):
        raise ValueError("dtype must be np.float64 or np.float32, got %r" % (dtype,)) from None


def dense_expression(toc, data, gene_count, normalization_method=0, dtype=np.float64, cell_ids=None, gene_local_ids=None, pitch=None):
    """getDenseExpressionMatrix (src/PythonModule.cpp:112-138) of a host CSR through em2_dense_expression -> ndarray
    [cells, gene_count] (the first gene_count columns of an array [cells, pitch] when pitch is given).  cell_ids: the rows of the
    CSR the result has, in that order; gene_local_ids: a GeneSet-*-LocalIds table for a CSR in global gene ids."""
    toc = np.ascontiguousarray(toc, dtype=np.uint64)
    data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
    csr_cells = len(toc) - 1
    if cell_ids is not None:
        cell_ids = np.ascontiguousarray(cell_ids, dtype=np.uint32)
    if gene_local_ids is not None:
        gene_local_ids = np.ascontiguousarray(gene_local_ids, dtype=np.uint32)
    cells = csr_cells if cell_ids is None else len(cell_ids)
    pitch = gene_count if pitch is None else pitch
    out = np.zeros((cells, pitch), dtype=dtype)
    check(load().em2_dense_expression(_ptr(toc), _ptr(data), csr_cells, _ptr(cell_ids) if cell_ids is not None else None, cells,
                                      _ptr(gene_local_ids) if gene_local_ids is not None else None,
                                      len(gene_local_ids) if gene_local_ids is not None else 0, gene_count, int(normalization_method),
                                      dense_element_type(dtype), _ptr(out), pitch))
    return out[:, :gene_count]


def dev_dense_expression(d_toc, d_data, cell_count, gene_count, normalization_method, d_out, pitch=None, row_begin=0, row_end=None,
                         d_cell_ids=None, d_gene_local_ids=None, global_gene_count=0, d_workspace=None, stream=None):
    """em2_dev_dense_expression on torch tensors: d_toc int64 [cells of the CSR + 1], d_data the (gene, count) records as bytes,
    d_out a float64 or float32 tensor of at least (row_end - row_begin) * pitch elements, which receives the rows
    [row_begin, row_end) of the result (cell_count rows: the CSR's, or those of d_cell_ids).  Runs on `stream` (a
    torch.cuda.Stream; default: the current one) and synchronises it."""
    import torch
    lib = load()
    row_end = cell_count if row_end is None else row_end
    pitch = gene_count if pitch is None else pitch
    if d_out.dtype not in (torch.float64, torch.float32):
        raise ValueError("d_out must be a float64 or float32 tensor")
    if not d_out.is_contiguous() or d_out.numel() < max(row_end - row_begin, 0) * pitch:
        raise ValueError("d_out must be contiguous and hold (row_end - row_begin) * pitch elements")
    element_type = DENSE_FLOAT64 if d_out.dtype == torch.float64 else DENSE_FLOAT32
    workspace_bytes = lib.em2_dev_dense_expression_workspace(max(row_end - row_begin, 0))
    if d_workspace is None:
        d_workspace = torch.empty(workspace_bytes, dtype=torch.uint8, device=d_out.device)
    stream = torch.cuda.current_stream() if stream is None else stream
    check(lib.em2_dev_dense_expression(d_toc.data_ptr(), d_data.data_ptr(), d_cell_ids.data_ptr() if d_cell_ids is not None else None,
                                       cell_count, d_gene_local_ids.data_ptr() if d_gene_local_ids is not None else None,
                                       global_gene_count, gene_count, int(normalization_method), row_begin, row_end, element_type,
                                       d_out.data_ptr(), pitch, d_workspace.data_ptr(), d_workspace.numel(), stream.cuda_stream))
    return d_out


# ---- colouring and drawing a laid-out graph (include/em2_lsh.h) ----
COLOR_NONE = 0x80000000
COLOR_BLACK = 0x40000000
NO_VALUE = float(np.finfo(np.float64).max)      # std::numeric_limits<double>::max(), the page's "no value"


def _optional_ids(ids, what):
    if ids is None:
        return None
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    if ids.ndim != 1:
        raise ValueError(what + " must be one-dimensional")
    return ids


def cell_similarities_to_cell(toc, data, gene_count, cell_id0, cell_ids, gene_local_ids=None):
    """em2_cell_similarities_to_cell -> float64 [len(cell_ids)]: computeCellSimilarity of cell_id0 against every listed cell."""
    toc = np.ascontiguousarray(toc, dtype=np.uint64)
    data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
    cell_ids = _optional_ids(cell_ids, "cell_ids")
    local = _optional_ids(gene_local_ids, "gene_local_ids")
    out = np.empty(len(cell_ids), dtype=np.float64)
    check(load().em2_cell_similarities_to_cell(_ptr(toc), _ptr(data), len(toc) - 1, _ptr(local) if local is not None else None,
                                               len(local) if local is not None else 0, gene_count, cell_id0, _ptr(cell_ids),
                                               len(cell_ids), _ptr(out)))
    return out


def cell_similarities_row_in_lds(gene_count):
    return bool(load().em2_cell_similarities_row_in_lds(gene_count))


def gene_expression_of_cells(toc, data, gene_count, gene_id, normalization_method, cell_ids, gene_local_ids=None):
    """em2_gene_expression_of_cells -> float32 [len(cell_ids)]: the normalized value of one gene in every listed cell."""
    toc = np.ascontiguousarray(toc, dtype=np.uint64)
    data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
    cell_ids = _optional_ids(cell_ids, "cell_ids")
    local = _optional_ids(gene_local_ids, "gene_local_ids")
    out = np.empty(len(cell_ids), dtype=np.float32)
    check(load().em2_gene_expression_of_cells(_ptr(toc), _ptr(data), len(toc) - 1, _ptr(local) if local is not None else None,
                                              len(local) if local is not None else 0, gene_count, gene_id, int(normalization_method),
                                              _ptr(cell_ids), len(cell_ids), _ptr(out)))
    return out


def spectral_colors(values, min_color_value=None, max_color_value=None):
    """em2_spectral_colors -> (rgb uint32 [n], range float64 [4] = minValue, maxValue, minColorValue, maxColorValue)."""
    values = np.ascontiguousarray(values, dtype=np.float64)
    rgb = np.empty(len(values), dtype=np.uint32)
    value_range = np.zeros(4, dtype=np.float64)
    check(load().em2_spectral_colors(_ptr(values), len(values), 0. if min_color_value is None else float(min_color_value),
                                     0. if max_color_value is None else float(max_color_value), int(min_color_value is not None),
                                     int(max_color_value is not None), _ptr(rgb), _ptr(value_range)))
    return rgb, value_range


def color_strings(rgb):
    """The page's colour string per packed colour: "" for none, "black", else "#rrggbb" from the same integers."""
    return ["" if c & COLOR_NONE else ("black" if c & COLOR_BLACK else "#%02x%02x%02x" % ((c >> 16) & 255, (c >> 8) & 255, c & 255))
            for c in np.asarray(rgb, dtype=np.uint32).tolist()]


def meta_data_number(value):
    raw = value if isinstance(value, bytes) else value.encode("utf-8", "surrogateescape")
    number = ctypes.c_double(0.)
    check(load().em2_meta_data_number(raw, len(raw), ctypes.byref(number)))
    return number.value


def graph_draw_long_edge_steps():
    return int(load().em2_graph_draw_long_edge_steps())


def graph_draw(x, y, edge_vertex0, edge_vertex1, size_pixels, x_view_box_center, y_view_box_center, view_box_half_size, vertex_radius,
               hide_edges=False, vertex_top=None, edge_hits=None):
    """em2_graph_draw -> (vertexTop, edgeHits), uint32 [S, S] each (row j, column i).  Arrays passed in are written in place."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    if x.shape != y.shape or x.ndim != 1:
        raise ValueError("x and y must be one-dimensional and of one length")
    v0 = np.ascontiguousarray(edge_vertex0, dtype=np.uint32)
    v1 = np.ascontiguousarray(edge_vertex1, dtype=np.uint32)
    if v0.shape != v1.shape or v0.ndim != 1:
        raise ValueError("edge_vertex0 and edge_vertex1 must be one-dimensional and of one length")
    size = int(size_pixels)
    shape = (size, size) if 1 <= size <= 8192 else (1, 1)          # (the entry reports a size out of range)
    if vertex_top is None:
        vertex_top = np.zeros(shape, dtype=np.uint32)
    if edge_hits is None:
        edge_hits = np.zeros(shape, dtype=np.uint32)
    for layer in (vertex_top, edge_hits):
        if layer.dtype != np.uint32 or layer.shape != shape or not layer.flags.c_contiguous:
            raise ValueError("a layer must be a C-contiguous uint32 [S, S] array")
    check(load().em2_graph_draw(len(x), _ptr(x), _ptr(y), len(v0), _ptr(v0), _ptr(v1), int(bool(hide_edges)), size & 0xffffffff,
                                float(x_view_box_center), float(y_view_box_center), float(view_box_half_size), float(vertex_radius),
                                _ptr(vertex_top), _ptr(edge_hits)))
    return vertex_top, edge_hits


def graph_compose(vertex_top, edge_hits, vertex_rgb=None, edge_shade=255):
    """em2_graph_compose -> uint8 [S, S, 4]."""
    vertex_top = np.ascontiguousarray(vertex_top, dtype=np.uint32)
    edge_hits = np.ascontiguousarray(edge_hits, dtype=np.uint32)
    if vertex_top.ndim != 2 or vertex_top.shape[0] != vertex_top.shape[1] or edge_hits.shape != vertex_top.shape:
        raise ValueError("the layers must be two [S, S] arrays")
    if vertex_rgb is None:
        vertex_rgb = np.zeros(int(vertex_top.max(initial=0)), dtype=np.uint32)
    vertex_rgb = np.ascontiguousarray(vertex_rgb, dtype=np.uint32)
    size = vertex_top.shape[0]
    rgba = np.empty((size, size, 4), dtype=np.uint8)
    check(load().em2_graph_compose(size, _ptr(vertex_top), _ptr(edge_hits), _ptr(vertex_rgb), len(vertex_rgb), int(edge_shade), _ptr(rgba)))
    return rgba


def _packed(strings):
    return b"".join(s.encode("utf-8", "surrogateescape") + b"\0" for s in strings)


def graph_write_svg(file_name, x, y, cell_ids, edge_vertex0, edge_vertex1, hide_edges, svg_size_pixels, x_view_box_center,
                    y_view_box_center, view_box_half_size, vertex_radius, edge_thickness, gene_set_name, vertex_colors=None,
                    vertex_groups=None, group_colors=None):
    """em2_graph_write_svg: CellGraph::writeSvg into file_name.  group_colors: {group: colour}, the reference's map; empty or
    None draws every vertex with its own colour (vertex_colors, a str per vertex, "" for none)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    cell_ids = np.ascontiguousarray(cell_ids, dtype=np.uint32)
    v0 = np.ascontiguousarray(edge_vertex0, dtype=np.uint32)
    v1 = np.ascontiguousarray(edge_vertex1, dtype=np.uint32)
    if not (len(x) == len(y) == len(cell_ids)) or len(v0) != len(v1):
        raise ValueError("the vertex arrays, and the edge arrays, must be of one length each")
    colors = None
    if vertex_colors is not None:
        if len(vertex_colors) != len(x):
            raise ValueError("vertex_colors must hold one string per vertex")
        colors = _packed(vertex_colors)
    group_colors = dict(group_colors or {})
    groups = None
    group_ids = np.asarray(sorted(group_colors), dtype=np.int32)
    group_strings = _packed([group_colors[g] for g in sorted(group_colors)])
    if group_colors:
        groups = np.ascontiguousarray(vertex_groups, dtype=np.uint32)
        if len(groups) != len(x):
            raise ValueError("vertex_groups must hold one group per vertex")
    check(load().em2_graph_write_svg(os.fsencode(file_name), len(x), _ptr(x), _ptr(y), _ptr(cell_ids), len(v0), _ptr(v0), _ptr(v1),
                                     int(bool(hide_edges)), float(svg_size_pixels), float(x_view_box_center), float(y_view_box_center),
                                     float(view_box_half_size), float(vertex_radius), float(edge_thickness), colors,
                                     len(colors) if colors is not None else 0, _ptr(groups) if groups is not None else None,
                                     len(group_ids), _ptr(group_ids), group_strings, len(group_strings),
                                     gene_set_name.encode("utf-8", "surrogateescape")))


PIE_COLOR_COUNT = 13          # the colour indices of a census: the twelve of the reference's palette, then "black"


def pie_census_wave_cells():
    return int(load().em2_pie_census_wave_cells())


def pie_census_take(handle):
    """The content of an em2_pie_census as a dict, and the handle freed: sliceOffsets uint64 [V + 1], sliceColor uint8,
    sliceCells uint32 and sliceFraction float64 per slice, waveVertexCount, and, from em2_matrix_pie_census, values (str) and
    valueCells (int) in the order that gave the values their colours."""
    lib = load()
    try:
        vertices, waves, slices = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
        check(lib.em2_pie_census_sizes(handle, ctypes.byref(vertices), ctypes.byref(slices), ctypes.byref(waves)))
        out = {"sliceOffsets": np.zeros(vertices.value + 1, dtype=np.uint64), "sliceColor": np.zeros(slices.value, dtype=np.uint8),
               "sliceCells": np.zeros(slices.value, dtype=np.uint32), "sliceFraction": np.zeros(slices.value, dtype=np.float64)}
        check(lib.em2_pie_census_get(handle, *[_ptr(out[key]) for key in ("sliceOffsets", "sliceColor", "sliceCells", "sliceFraction")]))
        out["waveVertexCount"] = waves.value
        count, size = ctypes.c_uint64(0), ctypes.c_uint64(0)
        check(lib.em2_pie_census_values_sizes(handle, ctypes.byref(count), ctypes.byref(size)))
        raw, cells = ctypes.create_string_buffer(max(1, size.value)), np.zeros(count.value, dtype=np.uint64)
        check(lib.em2_pie_census_values_get(handle, raw, _ptr(cells)))
        out["values"] = [v.decode("utf-8", "surrogateescape") for v in raw.raw[:size.value].split(b"\0")[:count.value]]
        out["valueCells"] = cells.tolist()
    finally:
        lib.em2_pie_census_free(handle)
    return out


def _pie_census_arrays(cell_offsets, cells, id_of_cell, color_of_value):
    cell_offsets = np.ascontiguousarray(cell_offsets, dtype=np.uint64)
    if cell_offsets.ndim != 1 or len(cell_offsets) < 1:
        raise ValueError("cell_offsets must hold vertexCount + 1 offsets")
    return (cell_offsets, np.ascontiguousarray(cells, dtype=np.uint32), np.ascontiguousarray(id_of_cell, dtype=np.uint32),
            np.ascontiguousarray(color_of_value, dtype=np.uint8))


def pie_census(cell_offsets, cells, id_of_cell, color_of_value):
    """em2_pie_census_create on host arrays -> the dict of pie_census_take."""
    cell_offsets, cells, id_of_cell, color_of_value = _pie_census_arrays(cell_offsets, cells, id_of_cell, color_of_value)
    handle = ctypes.c_void_p(None)
    check(load().em2_pie_census_create(len(cell_offsets) - 1, _ptr(cell_offsets), _ptr(cells), len(cells), _ptr(id_of_cell), len(id_of_cell),
                                       _ptr(color_of_value), len(color_of_value), ctypes.byref(handle)))
    return pie_census_take(handle)


def order_by_count(counts):
    """em2_order_by_count: the indices as std::sort leaves (index, count) under OrderPairsBySecondGreater, uint32."""
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    order = np.zeros(len(counts), dtype=np.uint32)
    check(load().em2_order_by_count(_ptr(counts), len(counts), _ptr(order)))
    return order


def signature_graph_random_colors(vertex_count):
    """em2_signature_graph_random_colors: colorRandom's colour per vertex as 0x00rrggbb, uint32."""
    rgb = np.zeros(int(vertex_count), dtype=np.uint32)
    check(load().em2_signature_graph_random_colors(len(rgb), _ptr(rgb)))
    return rgb


def pie_boundaries(slice_offsets, slice_fraction):
    """em2_pie_boundaries -> (boundaryX int32, boundaryY int32, largeArc uint8), one per slice."""
    slice_offsets = np.ascontiguousarray(slice_offsets, dtype=np.uint64)
    slice_fraction = np.ascontiguousarray(slice_fraction, dtype=np.float64)
    if len(slice_offsets) < 1 or int(slice_offsets[-1]) != len(slice_fraction):
        raise ValueError("slice_offsets must end at the number of slices")
    bx, by = np.zeros(len(slice_fraction), dtype=np.int32), np.zeros(len(slice_fraction), dtype=np.int32)
    arc = np.zeros(len(slice_fraction), dtype=np.uint8)
    check(load().em2_pie_boundaries(len(slice_offsets) - 1, _ptr(slice_offsets), _ptr(slice_fraction), _ptr(bx), _ptr(by), _ptr(arc)))
    return bx, by, arc


def graph_draw_pies_wave_radius():
    return float(load().em2_graph_draw_pies_wave_radius())


def graph_draw_pies(x, y, radius, edge_vertex0, edge_vertex1, size_pixels, x_view_box_center, y_view_box_center, view_box_half_size,
                    slice_offsets, boundary_x, boundary_y, large_arc, hide_edges=False, vertex_top=None, slice_top=None, edge_hits=None):
    """em2_graph_draw_pies -> (vertexTop, sliceTop, edgeHits), uint32 [S, S] each (row j, column i).  Arrays passed in are written
    in place."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    radius = np.ascontiguousarray(radius, dtype=np.float64)
    if not (x.shape == y.shape == radius.shape) or x.ndim != 1:
        raise ValueError("x, y and radius must be one-dimensional and of one length")
    v0 = np.ascontiguousarray(edge_vertex0, dtype=np.uint32)
    v1 = np.ascontiguousarray(edge_vertex1, dtype=np.uint32)
    if v0.shape != v1.shape or v0.ndim != 1:
        raise ValueError("edge_vertex0 and edge_vertex1 must be one-dimensional and of one length")
    slice_offsets = np.ascontiguousarray(slice_offsets, dtype=np.uint64)
    bx = np.ascontiguousarray(boundary_x, dtype=np.int32)
    by = np.ascontiguousarray(boundary_y, dtype=np.int32)
    arc = np.ascontiguousarray(large_arc, dtype=np.uint8)
    if len(slice_offsets) != len(x) + 1 or not (bx.shape == by.shape == arc.shape) or bx.ndim != 1:
        raise ValueError("slice_offsets must hold vertexCount + 1 offsets, and the three slice arrays must be of one length")
    size = int(size_pixels)
    shape = (size, size) if 1 <= size <= 8192 else (1, 1)          # (the entry reports a size out of range)
    layers = [np.zeros(shape, dtype=np.uint32) if layer is None else layer for layer in (vertex_top, slice_top, edge_hits)]
    for layer in layers:
        if layer.dtype != np.uint32 or layer.shape != shape or not layer.flags.c_contiguous:
            raise ValueError("a layer must be a C-contiguous uint32 [S, S] array")
    check(load().em2_graph_draw_pies(len(x), _ptr(x), _ptr(y), _ptr(radius), len(v0), _ptr(v0), _ptr(v1), int(bool(hide_edges)),
                                     size & 0xffffffff, float(x_view_box_center), float(y_view_box_center), float(view_box_half_size),
                                     _ptr(slice_offsets), len(bx), _ptr(bx), _ptr(by), _ptr(arc), *[_ptr(layer) for layer in layers]))
    return tuple(layers)


def signature_graph_write_svg(file_name, x, y, cell_counts, edge_vertex0, edge_vertex1, hide_edges=False, svg_size_pixels=500., x_shift=0.,
                              y_shift=0., zoom_factor=1., vertex_size_factor=1., edge_thickness_factor=1., slice_offsets=None,
                              slice_colors=None, slice_fraction=None):
    """em2_signature_graph_write_svg: SignatureGraph::writeSvg into file_name -> (xCenter, yCenter, halfViewBoxSize, pixelSize).
    slice_offsets None: every vertex is the black circle; else slice_colors holds a str and slice_fraction a float per slice."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    cell_counts = np.ascontiguousarray(cell_counts, dtype=np.uint64)
    v0 = np.ascontiguousarray(edge_vertex0, dtype=np.uint32)
    v1 = np.ascontiguousarray(edge_vertex1, dtype=np.uint32)
    if not (len(x) == len(y) == len(cell_counts)) or len(v0) != len(v1):
        raise ValueError("the vertex arrays, and the edge arrays, must be of one length each")
    offsets = fraction = colors = None
    if slice_offsets is not None:
        offsets = np.ascontiguousarray(slice_offsets, dtype=np.uint64)
        fraction = np.ascontiguousarray(slice_fraction, dtype=np.float64)
        if len(offsets) != len(x) + 1 or len(slice_colors) != len(fraction):
            raise ValueError("slice_offsets must hold vertexCount + 1 offsets, slice_colors and slice_fraction one entry per slice")
        colors = _packed(slice_colors)
    parameters = np.zeros(4, dtype=np.float64)
    check(load().em2_signature_graph_write_svg(os.fsencode(file_name), len(x), _ptr(x), _ptr(y), _ptr(cell_counts), len(v0), _ptr(v0),
                                               _ptr(v1), int(bool(hide_edges)), float(svg_size_pixels), float(x_shift), float(y_shift),
                                               float(zoom_factor), float(vertex_size_factor), float(edge_thickness_factor),
                                               _ptr(offsets) if offsets is not None else None, colors,
                                               len(colors) if colors is not None else 0,
                                               _ptr(fraction) if fraction is not None else None, _ptr(parameters)))
    return tuple(parameters.tolist())


def apply_gene_pairs_buffer():
    """EM2_GENE_PAIRS_BUFFER_MB (megabytes, default 4096): the device buffer findSimilarGenePairs0 passes its candidates
    through, handed to the library (em2_set_gene_pairs_buffer_mb) before every call."""
    text = os.environ.get("EM2_GENE_PAIRS_BUFFER_MB", "")
    try:
        megabytes = int(text) if text.strip() else GENE_PAIRS_BUFFER_MB_DEFAULT
    except ValueError:
        raise RuntimeError("EM2_GENE_PAIRS_BUFFER_MB must be a number of megabytes, not %r" % text) from None
    if megabytes < 0:
        raise RuntimeError("EM2_GENE_PAIRS_BUFFER_MB must not be negative")
    load().em2_set_gene_pairs_buffer_mb(megabytes)


def find_similar_gene_pairs0(toc, data, gene_count, normalization_method=2, k=100, similarity_threshold=0.2,
                             all_similarities=False):
    """findSimilarGenePairs0 (gene-gene correlations, all pairs) on a subset's host CSR -> (pairs [genes, k], usedCount),
    or (pairs, usedCount, r [genes, genes] float32) with all_similarities: the -Pairs and -GeneInfo content.  pairs["cell"]
    holds the partner's local gene id.  normalization_method: 0 none, 1 L1, 2 L2 (NormalizationMethod)."""
    toc = np.ascontiguousarray(toc, dtype=np.uint64)
    data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
    cell_count = len(toc) - 1
    pairs = np.zeros((gene_count, k), dtype=PAIR_DTYPE)
    used = np.zeros(gene_count, dtype=np.uint32)
    r = np.zeros((gene_count, gene_count), dtype=np.float32) if all_similarities else None
    apply_gene_pairs_buffer()
    check(load().em2_find_similar_gene_pairs0(_ptr(toc), _ptr(data), cell_count, gene_count, int(normalization_method), k,
                                              similarity_threshold, _ptr(pairs), _ptr(used),
                                              _ptr(r) if all_similarities else None))
    return (pairs, used, r) if all_similarities else (pairs, used)


def analyze_similar_pairs(toc, data, gene_count, pairs, used_count, global_cell_ids, csv_downsample, pairs_csv_path,
                          statistics_csv_path):
    """ExpressionMatrix::analyzeSimilarPairs on a subset's counts and a stored result (em2_analyze_similar_pairs) ->
    dict(sum0, sum1, sum2); writes the two csv files."""
    toc = np.ascontiguousarray(toc, dtype=np.uint64)
    data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
    pairs = np.ascontiguousarray(pairs, dtype=PAIR_DTYPE)
    used_count = np.ascontiguousarray(used_count, dtype=np.uint32)
    ids = np.ascontiguousarray(global_cell_ids, dtype=np.uint32)
    n = len(toc) - 1
    k = pairs.shape[1] if pairs.ndim == 2 else 0
    if len(used_count) != n or len(ids) != n or (pairs.ndim == 2 and pairs.shape[0] != n):
        raise ValueError("pairs, used_count and the cell ids must describe the cells of toc")
    out = {"sum0": np.zeros(200, dtype=np.uint64), "sum1": np.zeros(200, dtype=np.float64), "sum2": np.zeros(200, dtype=np.float64)}
    check(load().em2_analyze_similar_pairs(_ptr(toc), _ptr(data), n, gene_count, _ptr(pairs), _ptr(used_count), k, _ptr(ids),
                                           csv_downsample, os.fsencode(pairs_csv_path), os.fsencode(statistics_csv_path),
                                           _ptr(out["sum0"]), _ptr(out["sum1"]), _ptr(out["sum2"])))
    return out


def find_similar_pairs6(signatures, lsh_count, k, similarity_threshold, permutation_count, search_count,
                        permuted_bit_count=64, seed=231):
    """findSimilarPairs6 (the Charikar permutation search) on host signatures -> (pairs [cells, k], usedCount)."""
    signatures = np.ascontiguousarray(signatures, dtype=np.uint64)
    cell_count = signatures.shape[0]
    pairs = np.zeros((cell_count, k), dtype=PAIR_DTYPE)
    used = np.zeros(cell_count, dtype=np.uint32)
    check(load().em2_find_similar_pairs6(_ptr(signatures), cell_count, lsh_count, k, similarity_threshold, permutation_count,
                                         search_count, permuted_bit_count, seed, _ptr(pairs), _ptr(used)))
    return pairs, used


def find_similar_pairs7(signatures, lsh_count, k, similarity_threshold, lsh_slice_lengths, max_check, log2_bucket_count):
    signatures = np.ascontiguousarray(signatures, dtype=np.uint64)
    lengths = np.ascontiguousarray(lsh_slice_lengths, dtype=np.int32)
    cell_count = signatures.shape[0]
    pairs = np.zeros((cell_count, k), dtype=PAIR_DTYPE)
    used = np.zeros(cell_count, dtype=np.uint32)
    check(load().em2_find_similar_pairs7(_ptr(signatures), cell_count, lsh_count, k, similarity_threshold, _ptr(lengths),
                                         len(lengths), max_check, log2_bucket_count, _ptr(pairs), _ptr(used)))
    return pairs, used


# ---- device-pointer level (torch tensors supply the memory and the stream; this module never imports torch) ----

def dev_find_similar_pairs4_workspace(cell_count, row_count, lsh_count, k):
    return int(load().em2_dev_find_similar_pairs4_workspace(cell_count, row_count, lsh_count, k))


def dev_find_similar_pairs4_form(cell_count, row_count):
    """1 if the scan of this shape runs in its symmetric (each unordered pair once) form, else 0."""
    return int(load().em2_dev_find_similar_pairs4_form(cell_count, row_count))


def dev_find_similar_pairs4_form_for(cell_count, row_count, lsh_count):
    """The form a launch of row_count rows against cell_count columns of lsh_count-bit signatures takes: 0 ordered,
    1 symmetric, 3 symmetric on the matrix cores, 4 rows x all columns on the matrix cores."""
    return int(load().em2_dev_find_similar_pairs4_form_for(cell_count, row_count, lsh_count))


def dev_find_similar_pairs4_last_launch():
    """dict(form, scan_kernel_ms, wave_column_steps, inbox_entries, segments, full_row_cells, matrix_pairs,
    matrix_kernel_ms) of the last launch; form 0 ordered, 1 symmetric, 2 sharded symmetric, 3 symmetric on the matrix cores,
    4 rows x all columns on the matrix cores (a shard of the rows, or the fallback of a symmetric scan)."""
    v = np.zeros(9, dtype=np.float64)
    check(load().em2_dev_find_similar_pairs4_last_launch(_ptr(v), 9))
    return {"form": int(v[0]), "scan_kernel_ms": float(v[1]), "wave_column_steps": float(v[2]),
            "inbox_entries": float(v[3]), "segments": int(v[4]), "full_row_cells": int(v[5]),
            "matrix_pairs": float(v[6]), "matrix_kernel_ms": float(v[7]), "matrix_clock_ghz": float(v[8])}


# ---- em2_collectives (include/em2_lsh.h): the transport table of em2_dist_find_similar_pairs4_with ----
ALL_GATHER_FN = _c.CFUNCTYPE(_c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p)
ALL_REDUCE_MAX_I32_FN = _c.CFUNCTYPE(_c.c_int, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p)
ALL_TO_ALL_V_FN = _c.CFUNCTYPE(_c.c_int, _c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64), _c.c_void_p,
                               _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64), _c.c_void_p)


class Collectives(_c.Structure):
    _fields_ = [("context", _c.c_void_p), ("world", _c.c_int), ("rank", _c.c_int), ("all_gather", ALL_GATHER_FN),
                ("all_reduce_max_i32", ALL_REDUCE_MAX_I32_FN), ("all_to_all_v", ALL_TO_ALL_V_FN)]


DIST_STAGES = ("gather_signatures", "scan", "all_reduce", "exchange", "redistribute")


def dist_find_similar_pairs4_workspace(cell_count, lsh_count, k, rank, world):
    return int(load().em2_dist_find_similar_pairs4_workspace(cell_count, lsh_count, k, rank, world))


def dist_find_similar_pairs4_form(cell_count, lsh_count, k, world):
    return int(load().em2_dist_find_similar_pairs4_form(cell_count, lsh_count, k, world))


def dist_find_similar_pairs4(comm_or_table, local_sig_ptr, cell_count, lsh_count, k, similarity_threshold, all_sig_ptr, pairs_ptr,
                             used_ptr, workspace_ptr, workspace_bytes, stream, timed=False):
    """em2_dist_find_similar_pairs4 (comm_or_table: an ncclComm_t as int) or ..._with (a Collectives table); returns the
    per-stage wall ms as a dict when timed."""
    ms = (_c.c_double * len(DIST_STAGES))() if timed else None
    if isinstance(comm_or_table, Collectives):
        rc = load().em2_dist_find_similar_pairs4_with(_c.addressof(comm_or_table), local_sig_ptr, cell_count, lsh_count, k,
                                                      similarity_threshold, all_sig_ptr, pairs_ptr, used_ptr, workspace_ptr,
                                                      workspace_bytes, stream, ms)
    else:
        rc = load().em2_dist_find_similar_pairs4(comm_or_table, local_sig_ptr, cell_count, lsh_count, k, similarity_threshold,
                                                 all_sig_ptr, pairs_ptr, used_ptr, workspace_ptr, workspace_bytes, stream, ms)
    check(rc)
    return dict(zip(DIST_STAGES, ms)) if timed else None


# values[10] of em2_dev_find_similar_pairs5_last_launch (include/em2_lsh.h): the candidate filter that ran
FSP5_FILTER_FORMS = ("lane", "cooperative", "wide<4,4,true>", "wide<1,16,false>", "wide<1,8,false>", "wide<1,0,false>",
                     "wide<2,16,true>", "wide<2,16,false>", "wide<2,0,false>")


def dev_find_similar_pairs5_last_launch():
    """dict(gathered_candidates, cells, slice_count, batches, filter_ms, select_ms, distinct_candidates) of the last
    findSimilarPairs5 launch, and the forms it took: union_form (1 bitmap in LDS, 0 gather + segmented sort), union_passes,
    union_ids_per_pass, filter_form (one of FSP5_FILTER_FORMS), packed (the selection: 1 packed tiers, 0 whole entries)."""
    v = np.zeros(12, dtype=np.float64)
    check(load().em2_dev_find_similar_pairs5_last_launch(_ptr(v), 12))
    return {"gathered_candidates": float(v[0]), "cells": int(v[1]), "slice_count": int(v[2]), "batches": int(v[3]),
            "filter_ms": float(v[4]), "select_ms": float(v[5]), "distinct_candidates": float(v[6]),
            "union_form": int(v[7]), "union_passes": int(v[8]), "union_ids_per_pass": int(v[9]),
            "filter_form": FSP5_FILTER_FORMS[int(v[10])], "packed": int(v[11])}


def dev_release_scratch():
    """Frees the device scratch findSimilarPairs5 keeps between the calls of this process (include/em2_lsh.h)."""
    load().em2_dev_release_scratch()


def dev_find_similar_pairs4(sig_ptr, cell_count, row_begin, row_end, lsh_count, k, similarity_threshold,
                            pairs_ptr, used_ptr, workspace_ptr, workspace_bytes, stream):
    check(load().em2_dev_find_similar_pairs4(sig_ptr, cell_count, row_begin, row_end, lsh_count, k,
                                             similarity_threshold, pairs_ptr, used_ptr, workspace_ptr,
                                             workspace_bytes, stream))


def dev_fsp4_sharded_plan(cell_count, lsh_count, k, rank, world):
    """Layout of one rank's workspace for the sharded symmetric scan (see include/em2_lsh.h)."""
    v = np.zeros(12, dtype=np.uint64)
    check(load().em2_dev_fsp4_sharded_plan(cell_count, lsh_count, k, rank, world, _ptr(v), 12))
    names = ("eligible", "workspace_bytes", "snap_offset", "pool_offset", "pool_capacity", "gathered_offset",
             "gathered_capacity", "prefix_cells", "own_blocks", "blocks", "sorted_offset", "owner_shift")
    return {name: int(x) for name, x in zip(names, v)}


def dev_fsp4_sharded_phase(phase, sig_ptr, cell_count, lsh_count, k, similarity_threshold, rank, world, pairs_ptr,
                           used_ptr, workspace_ptr, workspace_bytes, gathered_count, stream):
    check(load().em2_dev_fsp4_sharded_phase(phase, sig_ptr, cell_count, lsh_count, k, similarity_threshold, rank, world,
                                            pairs_ptr, used_ptr, workspace_ptr, workspace_bytes, gathered_count, stream))


def dev_fsp4_sharded_status(cell_count, k, rank, world, workspace_ptr, stream):
    """(entries in this rank's pool, overflow flag); synchronises the stream."""
    used = ctypes.c_uint64(0)
    overflow = ctypes.c_uint32(0)
    check(load().em2_dev_fsp4_sharded_status(cell_count, k, rank, world, workspace_ptr, stream, ctypes.byref(used),
                                             ctypes.byref(overflow)))
    return int(used.value), int(overflow.value)


def dev_find_similar_pairs4_status(workspace_ptr, row_count, k, stream):
    """Synchronises the stream; raises if the scan reported an incomplete hand-off."""
    check(load().em2_dev_find_similar_pairs4_status(workspace_ptr, row_count, k, stream))


def dev_find_similar_pairs5(sig_ptr, cell_count, row_begin, row_end, lsh_count, k, similarity_threshold,
                            lsh_slice_length, bucket_overflow, pairs_ptr, used_ptr, stream):
    check(load().em2_dev_find_similar_pairs5(sig_ptr, cell_count, row_begin, row_end, lsh_count, k,
                                             similarity_threshold, lsh_slice_length, bucket_overflow, pairs_ptr,
                                             used_ptr, stream))


def dev_compute_signatures_workspace(cell_count, lsh_count):
    return int(load().em2_dev_compute_signatures_workspace(cell_count, lsh_count))


def dev_compute_signatures(toc_ptr, data_ptr, cell_count, gene_count, vectors_ptr, vector_aux_ptr, lsh_count,
                           sig_ptr, workspace_ptr, workspace_bytes, stream):
    check(load().em2_dev_compute_signatures(toc_ptr, data_ptr, cell_count, gene_count, vectors_ptr,
                                            vector_aux_ptr, lsh_count, sig_ptr, workspace_ptr, workspace_bytes,
                                            stream))


TIER_NAMES = ("exact", "float", "fixed16-float", "fixed16-integer")


def dev_compute_signatures_tier(workspace_ptr, cell_count, lsh_count, have_vector_aux=True):
    """Which first tier the last dev_compute_signatures call on this workspace ran (include/em2_lsh.h: EM2_TIER_*), by name."""
    tier = ctypes.c_int(-1)
    check(load().em2_dev_compute_signatures_tier(workspace_ptr, cell_count, lsh_count, 1 if have_vector_aux else 0, ctypes.byref(tier)))
    return TIER_NAMES[tier.value]


def dev_compute_signatures_listed(workspace_ptr, cell_count, lsh_count, have_vector_aux=True):
    """How far the tiers of the last dev_compute_signatures call on this workspace got (include/em2_lsh.h): the words listed for
    the float tier's word form, the words listed by a single bit, the entries left to the exact tier."""
    listed = (ctypes.c_uint32 * 3)()
    check(load().em2_dev_compute_signatures_listed(workspace_ptr, cell_count, lsh_count, 1 if have_vector_aux else 0, listed))
    return {"words": int(listed[0]), "bits": int(listed[1]), "exact": int(listed[2])}


def dev_vector_aux_bytes(gene_count, lsh_count):
    return int(load().em2_dev_vector_aux_bytes(gene_count, lsh_count))


def dev_prepare_vectors(vectors_ptr, gene_count, lsh_count, aux_ptr, stream):
    check(load().em2_dev_prepare_vectors(vectors_ptr, gene_count, lsh_count, aux_ptr, stream))


def dev_find_similar_pairs6(sig_ptr, cell_count, row_begin, row_end, lsh_count, k, similarity_threshold, permutation_count,
                            search_count, permuted_bit_count, seed, pairs_ptr, used_ptr, stream):
    check(load().em2_dev_find_similar_pairs6(sig_ptr, cell_count, row_begin, row_end, lsh_count, k, similarity_threshold,
                                             permutation_count, search_count, permuted_bit_count, seed, pairs_ptr, used_ptr,
                                             stream))


def dev_find_similar_pairs7(sig_ptr, cell_count, row_begin, row_end, lsh_count, k, similarity_threshold, lsh_slice_lengths,
                            max_check, log2_bucket_count, pairs_ptr, used_ptr, stream):
    """Rows [row_begin, row_end) of findSimilarPairs7 into pairs_ptr / used_ptr (row_end - row_begin rows); the slice
    lengths are a host sequence."""
    lengths = np.ascontiguousarray(lsh_slice_lengths, dtype=np.int32)
    check(load().em2_dev_find_similar_pairs7(sig_ptr, cell_count, row_begin, row_end, lsh_count, k, similarity_threshold,
                                             _ptr(lengths), len(lengths), max_check, log2_bucket_count, pairs_ptr, used_ptr,
                                             stream))


def dev_find_similar_pairs0_workspace(cell_count, row_count, gene_count, k):
    return int(load().em2_dev_find_similar_pairs0_workspace(cell_count, row_count, gene_count, k))


def dev_find_similar_pairs0(toc_ptr, data_ptr, cell_count, gene_count, row_begin, row_end, k, similarity_threshold, pairs_ptr,
                            used_ptr, lowest_index_ptr, lowest_ptr, workspace_ptr, workspace_bytes, stream):
    check(load().em2_dev_find_similar_pairs0(toc_ptr, data_ptr, cell_count, gene_count, row_begin, row_end, k,
                                             similarity_threshold, pairs_ptr, used_ptr, lowest_index_ptr, lowest_ptr,
                                             workspace_ptr, workspace_bytes, stream))
