"""ctypes binding of libsss.so: the C ABI declared in the headers of include/, one signature table per header
(``HEADERS`` below names them all).

The product path has NO CPU fallback: if the HIP library is missing or a call fails, this
module raises.  ``build()`` compiles the library in-tree with hipcc for gfx950.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from ctypes import c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsss.so")
CSRC = os.path.join(_HERE, "csrc")

_lib = None

# name -> (restype, argtypes); mirrors include/sss.h one to one
_SIGNATURES = {
    "sss_version": (c_int, []),
    "sss_last_error": (ctypes.c_char_p, []),
    "sss_normalize_rows": (c_int, [c_void_p, c_int64, c_int, c_int64, c_float, c_int, c_void_p]),
    "sss_row_norm_max": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "sss_f32_to_bf16": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "sss_ip_topk_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int, c_int, c_int]),
    "sss_ip_topk_state_bytes": (c_size_t, [c_int64]),
    "sss_ip_topk": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_int64, c_float,
                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p]),
    "sss_split_bf16": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "sss_ip_topk_split": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_int, c_int64, c_float,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t,
                                  c_void_p]),
    "sss_abs_max": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "sss_f16_shift": (c_int, [c_float]),
    "sss_scale_f16": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "sss_ip_topk_f16_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int, c_int]),
    "sss_f16_resid_max": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "sss_ip_topk_f16": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_float, c_int64, c_int, c_int, c_int64, c_float,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t,
                                c_void_p]),
    "sss_ip_topk_long_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int, c_int]),
    "sss_ip_topk_long": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_void_p, c_int, c_float, c_int64, c_int, c_int, c_int64,
                                 c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "sss_ip_topk_threshold_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int, c_int]),
    "sss_ip_topk_threshold": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_int, c_int, c_float, c_int64,
                                      c_int, c_int, c_int64, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                      c_void_p]),
    "sss_ip_topk_exhaustive_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "sss_ip_topk_exhaustive": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int,
                                       c_int64, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                       c_void_p]),
    "sss_ip_topk_exhaustive_lb": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int,
                                          c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "sss_range_search_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int, c_int]),
    "sss_range_search_count": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_void_p, c_int, c_int, c_float, c_int64, c_int, c_void_p,
                                       c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "sss_range_search_fill": (c_int, [c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "sss_range_search_exhaustive_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "sss_range_search_exhaustive_count": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_void_p,
                                                  c_void_p, c_void_p, c_size_t, c_void_p]),
    "sss_range_search_exhaustive_fill": (c_int, [c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                                 c_void_p, c_size_t, c_void_p]),
    "sss_topk_merge": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int64, c_int, c_void_p, c_void_p,
                               c_void_p]),
    "sss_scan_boot_expired": (c_int, [c_int]),
    "sss_profile_enable": (c_int, [c_int]),
    "sss_profile_read": (c_int, [c_void_p, c_void_p]),
    "sss_gather_rows": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p]),
    "sss_gather_concat_rows": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_int, c_int, c_int64, c_void_p, c_int64,
                                       c_void_p]),
    "sss_linear": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64,
                           c_int, c_int, c_void_p]),
    "sss_gat_aggregate": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                                  c_int64, c_int, c_void_p, c_int, c_int64, c_void_p, c_int64, c_void_p]),
    "sss_csr_weighted_sum": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int,
                                     c_void_p, c_int64, c_void_p]),
    "sss_gru_combine": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p,
                                c_int64, c_int64, c_int, c_void_p, c_int64, c_void_p]),
    "sss_pool_expand": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int,
                                c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    "sss_segment_pool": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p,
                                 c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "sss_segment_ptr": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "sss_pack_sign_bits": (c_int, [c_void_p, c_int64, c_int, c_int64, c_void_p, c_int, c_void_p]),
    "sss_hamming_topk_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "sss_hamming_topk_capacity": (c_int, [c_int64, c_int64]),
    "sss_hamming_topk": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_size_t, c_void_p]),
    "sss_hamming_topk_exhaustive_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "sss_hamming_topk_exhaustive": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int64,
                                            c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "sss_graph_scratch_ints": (c_size_t, [c_int64]),
    "sss_graph_counts": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sss_graph_fill": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "sss_knn_item_vote": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int64, c_int64, c_int,
                                  c_void_p, c_void_p, c_void_p, c_void_p]),
    "sss_linear_grouped": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "sss_hetero_layer_update": (c_int, [c_void_p, c_void_p]),
    "sss_pool_expand_mean": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                     c_int64, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "sss_pool_attention": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                   c_int64, c_int64, c_int, c_int, c_float, c_int, c_void_p, c_int64, c_void_p]),
    "sss_pool_attention_tab": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_float,
                                       c_void_p, c_int64, c_void_p]),
    "sss_csr_mean": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p]),
    "sss_segment_reduce": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_int64, c_void_p]),
    "sss_attention_dot_pool": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p]),
}

# include/sss_sparse.h one to one (the sparse session index: its own header, bound from the same library)
_SPARSE_SIGNATURES = {
    "sss_session_vectors_count": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "sss_session_vectors_fill": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, ctypes.c_double, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p]),
    "sss_sparse_topk_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "sss_sparse_topk": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int64,
                                c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}

# include/sss_l2.h one to one (L2 top-k on the matrix-core scans)
_L2_SIGNATURES = {
    "sss_l2_row_bias": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "sss_l2_topk_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int, c_int, c_int]),
    "sss_l2_topk": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_int64, c_int, c_int, c_int64,
                            c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p]),
    "sss_l2_topk_threshold_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int, c_int]),
    "sss_l2_topk_threshold": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_int64, c_int,
                                      c_int, c_int64, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}

# include/sss_l2_long.h one to one (L2 top-k of long float32 rows on the K-tiled scan)
_L2_LONG_SIGNATURES = {
    "sss_l2_topk_long_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int]),
    "sss_l2_topk_long": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_float, c_void_p, c_int64, c_int, c_int, c_int64,
                                 c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}

# include/sss_pad.h one to one (scans at the next supported width for float32 rows of any width d % 4 == 0)
_PAD_SIGNATURES = {
    "sss_pad_rows_f32": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "sss_pad_scale_f16": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p]),
    "sss_pad_split_bf16": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "sss_pad_f16_resid_max": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p]),
    "sss_pad_topk_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int, c_int, c_int, c_int]),
    "sss_pad_topk": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_int64, c_int, c_int, c_int,
                             c_int64, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t,
                             c_void_p]),
    "sss_pad_topk_threshold_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int, c_int, c_int]),
    "sss_pad_topk_threshold": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_int64,
                                       c_int, c_int, c_int, c_int64, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                       c_void_p]),
}

# include/sss_graph.h one to one (the graph builder with ignore_query and the last-click outputs)
GRAPH_IGNORE_QUERY = 1      # SSS_GRAPH_IGNORE_QUERY
_GRAPH_SIGNATURES = {
    "sss_graph_counts_ex": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sss_graph_fill_ex": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p]),
}

# include/sss_eval.h one to one (scoring a search result: pair overlaps of item sets and their per-query sums)
_EVAL_SIGNATURES = {
    "sss_item_overlap": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int64, c_void_p, c_void_p,
                                 c_void_p, c_void_p]),
    "sss_overlap_metrics": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p, c_void_p, c_void_p]),
}

# include/sss_jaccard.h one to one (ground truth: exact item-set Jaccard top-k and band counts over the whole corpus;
# `edges` of sss_jaccard_bands is the one HOST pointer of the ABI)
_JACCARD_SIGNATURES = {
    "sss_jaccard_topk_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "sss_jaccard_topk": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p,
                                 c_void_p, c_size_t, c_void_p]),
    "sss_jaccard_bands": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int64, c_void_p,
                                  c_void_p, c_void_p]),
}

# include/sss_ptype.h one to one (ground truth under the product-type kind: type bags, their exact top-k, band counts and
# pair scores; `edges` of sss_ptype_bands is a HOST pointer, as sss_jaccard_bands')
_PTYPE_SIGNATURES = {
    "sss_type_bags_count": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "sss_type_bags_fill": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p]),
    "sss_ptype_topk_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "sss_ptype_topk": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int64,
                               c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "sss_ptype_bands": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int64,
                                c_void_p, c_void_p, c_void_p]),
    "sss_ptype_pair_scores": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int,
                                      c_int64, c_void_p, c_void_p, c_void_p]),
}

# include/sss_hgt.h one to one (the HGT encoder: HGTConv's attention aggregation on CSR by target and its skip connection)
_HGT_SIGNATURES = {
    "sss_hgt_aggregate": (c_int, [c_void_p, c_void_p]),
    "sss_hgt_skip": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_float, c_int64, c_int, c_void_p]),
}

# include/sss_text.h one to one (the query text encoder: token embedding, attention inside packed sequences, add + LayerNorm)
_TEXT_SIGNATURES = {
    "sss_text_embed": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p, c_int64,
                               c_void_p, c_void_p]),
    "sss_seq_attention": (c_int, [c_void_p, c_void_p]),
    "sss_add_layernorm": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_float, c_int64, c_int, c_void_p, c_int64,
                                  c_void_p]),
}

# include/sss_bert.h one to one (the node text encoder: BERT's embedding stage; the rest of its forward is bound above)
_BERT_SIGNATURES = {
    "sss_bert_embed": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_float, c_int64, c_int, c_void_p, c_int64, c_void_p, c_void_p]),
}


# header of include/ -> its signature table: what lib() binds, and every *_symbols() view below
HEADERS = {
    "sss.h": _SIGNATURES,
    "sss_sparse.h": _SPARSE_SIGNATURES,
    "sss_l2.h": _L2_SIGNATURES,
    "sss_l2_long.h": _L2_LONG_SIGNATURES,
    "sss_pad.h": _PAD_SIGNATURES,
    "sss_graph.h": _GRAPH_SIGNATURES,
    "sss_eval.h": _EVAL_SIGNATURES,
    "sss_jaccard.h": _JACCARD_SIGNATURES,
    "sss_ptype.h": _PTYPE_SIGNATURES,
    "sss_hgt.h": _HGT_SIGNATURES,
    "sss_text.h": _TEXT_SIGNATURES,
    "sss_bert.h": _BERT_SIGNATURES,
}


class LinearProblem(ctypes.Structure):
    """``sss_linear_problem`` of include/sss.h."""
    _fields_ = [("x", c_void_p), ("ldx", c_int64), ("ids", c_void_p), ("table", c_void_p), ("xcopy", c_void_p),
                ("ld_xcopy", c_int64), ("w", c_void_p), ("ldw", c_int64), ("bias", c_void_p), ("y", c_void_p),
                ("ldy", c_int64), ("n", c_int64), ("m", c_int32), ("act", c_int32), ("post_scale", c_void_p), ("post_shift", c_void_p)]


def linear_problem(x, w, bias, y, n, m, act=0, post=None, ids=None, table=None, xcopy=None):
    """One problem of ``sss_linear_grouped``: ``y[:n, :m] = act(x w^T + bias)`` on 2-D device tensors (row strides are taken
    from them), ``post = (scale, shift)`` the second epilogue stage.  Gather mode: ``x = None``, ``ids`` / ``table`` the
    rows' source and ``xcopy`` (optional) where the gathered rows are also written."""
    ptr = lambda t: 0 if t is None else t.data_ptr()
    ld = lambda t: 0 if t is None else t.stride(0)
    return LinearProblem(x=ptr(x), ldx=ld(x), ids=ptr(ids), table=ptr(table), xcopy=ptr(xcopy), ld_xcopy=ld(xcopy),
                         w=w.data_ptr(), ldw=w.stride(0), bias=ptr(bias), y=y.data_ptr(), ldy=y.stride(0), n=n, m=m, act=act,
                         post_scale=0 if post is None else post[0].data_ptr(),
                         post_shift=0 if post is None else post[1].data_ptr())


def pad32(n):
    """``n`` rounded up to the multiple of 32 that the GEMM's K has to be."""
    return (n + 31) // 32 * 32


class GraphOut(ctypes.Structure):
    """``sss_graph_out`` of include/sss.h."""
    _fields_ = [(n, c_void_p) for n in ("q_x", "q_batch", "q_pos", "p_x", "p_batch", "p_cnt", "rowptr_qp", "col_qp",
                                        "rowptr_pq", "col_pq", "rowptr_pp", "col_pp", "w_pp", "src_row", "pos_id")]


class LayerArgs(ctypes.Structure):
    """``sss_layer_args`` of include/sss.h."""
    _fields_ = [("yp", c_void_p), ("ld_yp", c_int64), ("yq", c_void_p), ("ld_yq", c_int64), ("h", c_int32), ("d_x", c_int32),
                ("rowptr_qp", c_void_p), ("col_qp", c_void_p), ("rowptr_pp", c_void_p), ("col_pp", c_void_p),
                ("w_pp", c_void_p), ("bias_qp", c_void_p), ("b_ih", c_void_p),
                ("xin_p", c_void_p), ("ld_xin", c_int64), ("out_p", c_void_p), ("ld_out_p", c_int64), ("np", c_int64),
                ("rowptr_pq", c_void_p), ("col_pq", c_void_p), ("bias_pq", c_void_p),
                ("out_q", c_void_p), ("ld_out_q", c_int64), ("nq", c_int64), ("n_self_loop", c_int64),
                ("row_p", c_void_p), ("row_q", c_void_p), ("x0_p", c_void_p), ("ld_x0_p", c_int64),
                ("xq_table", c_void_p), ("ld_xq", c_int64), ("x0_q", c_void_p), ("ld_x0_q", c_int64)]


class HgtSlot(ctypes.Structure):
    """``sss_hgt_slot`` of include/sss_hgt.h."""
    _fields_ = [("k", c_void_p), ("ld_k", c_int64), ("v", c_void_p), ("ld_v", c_int64), ("rowptr", c_void_p), ("col", c_void_p)]


class HgtArgs(ctypes.Structure):
    """``sss_hgt_args`` of include/sss_hgt.h."""
    _fields_ = [("q", c_void_p), ("ld_q", c_int64), ("slot", HgtSlot * 2), ("n_slots", c_int32), ("n_dst", c_int64),
                ("heads", c_int32), ("head_dim", c_int32), ("gelu", c_int32), ("out", c_void_p), ("ld_out", c_int64)]


class SeqAttentionArgs(ctypes.Structure):
    """``sss_seq_attention_args`` of include/sss_text.h."""
    _fields_ = [("qkv", c_void_p), ("ld_qkv", c_int64), ("ptr", c_void_p), ("key_ok", c_void_p), ("n_rows", c_int64),
                ("n_seq", c_int64), ("heads", c_int32), ("head_dim", c_int32), ("max_len", c_int32), ("out", c_void_p),
                ("ld_out", c_int64)]


def exported_symbols():
    return sorted(HEADERS["sss.h"])


def sparse_symbols():
    """The entry points of include/sss_sparse.h."""
    return sorted(HEADERS["sss_sparse.h"])


def l2_symbols():
    """The entry points of include/sss_l2.h."""
    return sorted(HEADERS["sss_l2.h"])


def l2_long_symbols():
    """The entry points of include/sss_l2_long.h."""
    return sorted(HEADERS["sss_l2_long.h"])


def pad_symbols():
    """The entry points of include/sss_pad.h."""
    return sorted(HEADERS["sss_pad.h"])


def graph_symbols():
    """The entry points of include/sss_graph.h."""
    return sorted(HEADERS["sss_graph.h"])


def eval_symbols():
    """The entry points of include/sss_eval.h."""
    return sorted(HEADERS["sss_eval.h"])


def jaccard_symbols():
    """The entry points of include/sss_jaccard.h."""
    return sorted(HEADERS["sss_jaccard.h"])


def ptype_symbols():
    """The entry points of include/sss_ptype.h."""
    return sorted(HEADERS["sss_ptype.h"])


def hgt_symbols():
    """The entry points of include/sss_hgt.h."""
    return sorted(HEADERS["sss_hgt.h"])


def text_symbols():
    """The entry points of include/sss_text.h."""
    return sorted(HEADERS["sss_text.h"])


def bert_symbols():
    """The entry points of include/sss_bert.h."""
    return sorted(HEADERS["sss_bert.h"])


def build(verbose: bool = False) -> str:
    """Compile libsss.so for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j4"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building libsss.so failed:\n" + res.stdout[-4000:] + res.stderr[-4000:])
    if verbose:
        print(res.stdout)
    return LIB_PATH


def lib():
    """The loaded library; raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP extension is not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C "
                "sessionsimilaritysearch_amd/csrc`). There is no CPU fallback.")
        h = ctypes.CDLL(LIB_PATH)
        for table in HEADERS.values():
            for name, (res, args) in table.items():
                fn = getattr(h, name)      # AttributeError if the .so lacks a declared symbol
                fn.restype, fn.argtypes = res, args
        _lib = h
    return _lib


class SssError(RuntimeError):
    pass


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().sss_last_error()
        raise SssError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


def stream_ptr(device=None):
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def require_cuda(t, name, dtype=None):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise SssError(f"{name} must be a CUDA (HIP) tensor")
    if dtype is not None and t.dtype != dtype:
        raise SssError(f"{name} must have dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise SssError(f"{name} must be contiguous")
    return t
