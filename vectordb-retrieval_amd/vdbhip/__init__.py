"""vdbhip -- MI355X-native exact / IVF k-NN behind the vectordb-retrieval plugin API.

Importing the package does not touch the GPU and does not import torch; the shared library
(libvdbhip.so, hand-written HIP for gfx950) is dlopen'ed on first use and there is no CPU fallback.
"""
from .plugin_api import (ALGORITHM_REGISTRY, INDEXER_REGISTRY, SEARCHER_REGISTRY, BaseAlgorithm, BaseIndexer,
                         BaseSearcher, CompositeAlgorithm, IndexArtifact, get_algorithm_instance, get_indexer_class,
                         get_searcher_class, register_algorithm, register_indexer, register_searcher)
from .algorithms import HipBruteForceIndexer, HipExactSearch, HipLinearSearcher, rerank_candidates
from .index import FlatIndex, merge_packed_partials_device, merge_partials_device
from .ivf import HipApproximateSearch, HipIVFIndexer, HipIVFSearcher, IVFFlatIndex, IVFI8Index, IVFSQ8Index, parse_index_key
from .ivf_pq import HipIVFPQIndexer, HipIVFPQSearch, IVFPQIndex, parse_ivfpq_key
from .knng import HipKnnGraphIndexer, HipKnnGraphSearch, HipKnnGraphSearcher, KnnGraphIndex
from .lsh import HipLSHIndexer, HipLSHSearcher, make_projection
from .lsh_tables import HipLSHTableIndexer, HipLSHTables, HipLSHTableSearcher, make_tables
from .pq import HipPQIndexer, HipPQSearch, HipPQSearcher, PQIndex, parse_pq_key
from . import sharded
from .sharded import HipShardedApproximateSearch, HipShardedExactSearch, shard_bounds

__all__ = [
    "ALGORITHM_REGISTRY", "INDEXER_REGISTRY", "SEARCHER_REGISTRY", "BaseAlgorithm", "BaseIndexer", "BaseSearcher",
    "CompositeAlgorithm", "IndexArtifact", "get_algorithm_instance", "get_indexer_class", "get_searcher_class",
    "register_algorithm", "register_indexer", "register_searcher", "HipExactSearch", "HipBruteForceIndexer",
    "HipLinearSearcher", "rerank_candidates", "FlatIndex", "merge_partials_device", "merge_packed_partials_device",
    "HipApproximateSearch", "HipIVFIndexer", "HipIVFSearcher", "IVFFlatIndex", "IVFI8Index", "IVFSQ8Index", "parse_index_key",
    "HipIVFPQIndexer", "HipIVFPQSearch", "IVFPQIndex", "parse_ivfpq_key",
    "HipKnnGraphIndexer", "HipKnnGraphSearcher", "HipKnnGraphSearch", "KnnGraphIndex",
    "HipLSHIndexer", "HipLSHSearcher", "make_projection", "HipLSHTableIndexer", "HipLSHTableSearcher", "HipLSHTables",
    "make_tables", "HipPQIndexer", "HipPQSearcher", "HipPQSearch", "PQIndex",
    "parse_pq_key", "HipShardedExactSearch",
    "HipShardedApproximateSearch", "shard_bounds", "sharded",
]
