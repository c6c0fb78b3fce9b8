"""MI355X-native session-similarity retrieval hot path.

Drop-in surface of the reference's path:
  normalize, build_index, FlatIndex (f32 / bf16 / f16 / i8), quantize_i8
                                                  (index.py     <- test_amazon_filterd.py / util_amazon_filtered.py)
  BinaryFlatIndex, pack_sign_bits                 (index.py     <- fine_tune_ours.py IndexBinaryFlat branch)
  SessionEncoder (+ prepare_actions), session_fold_weights
                                                  (encoder.py   <- model/model.py UnifyPoolingGraphLevelEncoder,
                                                                  util_amazon_filtered.sequence_to_graph)
  get_prediction_by_knn, get_p_r, SessionItems    (retrieval.py <- test_amazon_filterd.py:59-85)
  HeteroSAGE, GraphPooling, AttentionPooling, ... (variants.py  <- model/gnn.py, model/model.py variants)
  HGT, hgt_fold_weights                           (variants.py  <- model/gnn.py HGT: the two-tower model's encoder)
  SparseSessionIndex, session_vectors, find_K_sparse_dense
                                                  (sparse.py    <- test_amazon_filterd.py SKNN / STAN item-vector baselines)
  evaluate, query_parts, item_overlap, get_*_jaccard, get_*_recall, get_*_map, get_ave_score, get_recall
                                                  (evaluation.py <- test_amazon_filterd.py:226-382, 443-450 and
                                                                  fine_tune_ours.py:42-97, the item-set metrics of a result)
  JaccardIndex, mine_triples, neighbourhood_recall
                                                  (jaccard.py   <- fine_tune_ours.py get_score :42-55 over the whole corpus,
                                                                  the triple mining :187-235: the ground truth)
  ProductTypeIndex, type_bags                     (product_types.py <- fine_tune_ours.py get_score :66-85, the kind of
                                                                  CFG.sim_type = 'all_product_type_score', over the whole corpus)
  NodeTextTransformer, pack_tokens, text_fold_weights, TokenRows
                                                  (text.py      <- model/NodeEmbedding.py NodeTextTransformer: the two-tower
                                                                  model's query text encoder, eval mode)
  BertNodeEncoder, bert_fold_weights, bert_pack_rows, BertRows
                                                  (text.py      <- model/NodeEmbedding.py PretrainedQAEAEncoder: the deployed
                                                                  model's node text encoder, BERT + masked mean + Linear)
  StringTable, StringSequences, query_sequences, title_sequences, sequence_parts, seq_pair_scores, get_query_metric
                                                  (strings.py   <- fine_tune_ours.py get_score :56-65, the Levenshtein.seqratio
                                                                  kinds, and test_amazon_filterd.py get_query_metric :416-441)
  ShardedFlatIndex, ShardedBinaryIndex, ShardedSparseIndex, ShardedJaccardIndex, ShardedProductTypeIndex
                                                  (distributed.py: corpus row-sharded over RCCL)
  SessionBatch, build_batch, synthetic_actions    (sessions.py  <- sequence_to_graph + Batch.from_data_list, host side)
  CatalogueHead, CatalogueLoss, get_next_product_asin_accuracy, get_all_product_asin_accuracy, get_next_product_asin_loss,
  get_all_product_asin_loss                       (catalogue.py <- train_subsession_embedding.py:271-339 and
                                                                  train_session_embedding.py:87-: the model's own item
                                                                  prediction over the catalogue and its validation loss)
  WordPieceTokenizer, TokenTable, Tokens          (wordpiece.py <- util_amazon_filtered.py:19-20, 120-121: the BERT tokenizer
                                                                  calls of sequence_to_graph, over a StringTable)
"""
from ._lib import SssError, build, exported_symbols, lib  # noqa: F401

__all__ = ["SssError", "build", "exported_symbols", "lib", "SessionVectors", "SparseSessionIndex", "session_vectors",
           "find_K_sparse_dense", "QueryParts", "query_parts", "item_overlap", "evaluate", "get_cur_jaccard", "get_future_jaccard",
           "get_all_jaccard", "get_cur_recall", "get_all_recall", "get_future_recall", "get_future_map", "get_cur_map", "get_all_map",
           "get_ave_score", "get_recall"]
_EVALUATION = frozenset(__all__[8:])
_JACCARD = ("JaccardIndex", "mine_triples", "neighbourhood_recall")
__all__ += list(_JACCARD)
_PTYPE = ("ProductTypeIndex", "type_bags")
__all__ += list(_PTYPE)
_ENCODER = ("session_fold_weights",)
__all__ += list(_ENCODER)
_HGT = ("HGT", "hgt_fold_weights")
__all__ += list(_HGT)
_TEXT = ("NodeTextTransformer", "pack_tokens", "text_fold_weights", "TokenRows", "BertNodeEncoder", "bert_fold_weights",
         "bert_pack_rows", "BertRows")
__all__ += list(_TEXT)
_STRINGS = ("StringTable", "StringSequences", "SequenceParts", "query_sequences", "title_sequences", "sequence_parts",
            "seq_pair_scores", "seq_query_metric", "get_query_metric")
__all__ += list(_STRINGS)
_CATALOGUE = ("CatalogueHead", "CatalogueLoss", "get_next_product_asin_accuracy", "get_all_product_asin_accuracy",
              "get_next_product_asin_loss", "get_all_product_asin_loss")
__all__ += list(_CATALOGUE)
_WORDPIECE = ("WordPieceTokenizer", "TokenTable", "Tokens")
__all__ += list(_WORDPIECE)


def __getattr__(name):
    # the sparse session index, re-exported lazily: importing it pulls in torch, which `build()` does not need
    if name in ("SessionVectors", "SparseSessionIndex", "session_vectors", "find_K_sparse_dense"):
        from . import sparse
        return getattr(sparse, name)
    if name in _EVALUATION:                              # scoring a result: lazily, for the same reason
        from . import evaluation
        return getattr(evaluation, name)
    if name in _JACCARD:                                 # the ground-truth index: lazily, for the same reason
        from . import jaccard
        return getattr(jaccard, name)
    if name in _PTYPE:                                   # the product-type index: lazily, for the same reason
        from . import product_types
        return getattr(product_types, name)
    if name in _ENCODER:                                 # the session encoder's fold: lazily, for the same reason
        from . import encoder
        return getattr(encoder, name)
    if name in _HGT:                                     # the HGT encoder: lazily, for the same reason
        from . import variants
        return getattr(variants, name)
    if name in _TEXT:                                    # the query text encoder: lazily, for the same reason
        from . import text
        return getattr(text, name)
    if name in _STRINGS:                                 # the string metrics of a result: lazily, for the same reason
        from . import strings
        return getattr(strings, name)
    if name in _CATALOGUE:                               # the catalogue heads: lazily, for the same reason
        from . import catalogue
        return getattr(catalogue, name)
    if name in _WORDPIECE:                               # the tokenizer: lazily, for the same reason
        from . import wordpiece
        return getattr(wordpiece, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
