"""The reference's /vectors routes over the MI355X store.

Same paths, request bodies, response shapes and score formatting as
/root/reference/api/routes/vectors.py, so its SDKs (sdk/python/mlx_vector_client.py:346-404)
and HTTP scripts work unchanged:

  POST /vectors/add           {user_id, model_id, vectors, metadata}       (:163-207)
  POST /vectors/query         {user_id, model_id, query, k, filter_metadata} (:211-270)
  POST /vectors/batch_query   {user_id, model_id, queries, k[, filter_metadata]}            (:272-330)
  GET  /vectors/count, /vectors/stats, /vectors/health                     (:332-388)
  POST /vectors/delete        {user_id, model_id, filter_metadata} -> {deleted}: the call the
                              SDK's delete_vectors_by_metadata makes
                              (sdk/python/mlx_vector_db_client.py:292-303); the reference
                              server has no such route

Differences, on purpose:
  * /batch_query works: the reference calls a ``store.batch_query`` that does not exist
    and always answers 500 (:291, :328-330); here the store's batched device search runs
    (service/optimized_vector_store.py ``batch_query``, which returns distances because
    this route scores cosine as ``max(0, 1 - dist)``, :300-306).
  * Stores are created lazily per (user, model) as in ``VectorStoreManager.get_store``
    (:48-71), under ``$VECTOR_STORE_BASE`` (default the reference's
    ``~/.team_mind_data/vector_stores``); the store config (metric, devices) comes from a
    factory the app may replace.

Scores (S12, :236-258): cosine ``similarity = raw, distance = 1 - raw``; euclidean
``distance = raw, similarity = 1 / (1 + distance)``; each result has ``rank`` and no
``index``.  Every store call runs on a 4-thread executor, like the reference (:43).
"""
from __future__ import annotations

import asyncio
import logging
import os
import secrets
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import Any, Callable, Dict, List, Optional, Union

from fastapi import APIRouter, Depends, HTTPException, Security
from fastapi.security import HTTPAuthorizationCredentials, HTTPBearer
from pydantic import BaseModel, Field, model_validator

from service.filter_ops import FilterError
from service.optimized_vector_store import GROUP_MAX_K, GROUP_MAX_SIZE, MLXVectorStore, MLXVectorStoreConfig

logger = logging.getLogger(__name__)


# ---- request / response models (service/models.py:34-61, api/routes/vectors.py:147-161) ----
class VectorAddRequest(BaseModel):
    user_id: str
    model_id: str
    vectors: List[List[float]] = Field(..., description="List of vectors to add")
    metadata: List[Dict[str, Any]] = Field(..., description="Metadata for each vector")

    @model_validator(mode="after")
    def validate_same_length(self):
        if len(self.vectors) != len(self.metadata):
            raise ValueError("Vectors and metadata must have the same length")
        return self


class VectorQuery(BaseModel):
    user_id: str
    model_id: str
    query: List[float] = Field(..., description="Query vector")
    k: int = Field(default=10, ge=1, le=1000)
    filter_metadata: Optional[Dict[str, Any]] = Field(default=None, description="Metadata filter")


class VectorMMRQuery(VectorQuery):
    """/vectors/query's body plus the two MMR settings: ``k`` rows picked from the best ``fetch_k``
    (null: min(200, max(4 k, 20))), each maximising ``lambda_mult`` * relevance - (1 - ``lambda_mult``)
    * its greatest similarity to a row picked before.  The store checks the limits (k and fetch_k at
    most 200, fetch_k >= k, lambda_mult in [0, 1]); a value outside them is a 400."""
    fetch_k: Optional[int] = Field(default=None, description="Candidates the rows are picked from")
    lambda_mult: float = Field(default=0.5, description="1 = relevance only, 0 = diversity only")


class VectorFusedQuery(BaseModel):
    """One ranked list from several query vectors (paraphrases of a question, the question plus a
    hypothetical answer, ...): each vector's best ``fetch_k`` rows (null: min(200, max(k, 4 k))) are
    fused per row, ``fusion`` "rrf": the sum of ``weights[l] / (rrf_c + rank)`` over the lists holding
    it, "max": its best match to any of the vectors.  The store checks the limits (at most 16
    vectors, k and fetch_k at most 200, fetch_k >= k, weights finite and >= 0 and only with "rrf");
    a value outside them is a 400."""
    user_id: str
    model_id: str
    queries: List[List[float]] = Field(..., description="The query vectors fused into one list")
    k: int = Field(default=10, description="Rows returned")
    fusion: str = Field(default="rrf", description='"rrf" (weighted reciprocal rank) or "max" (best match to any)')
    weights: Optional[List[float]] = Field(default=None, description="One weight per query vector (rrf only)")
    fetch_k: Optional[int] = Field(default=None, description="Rows fetched per query vector")
    rrf_c: float = Field(default=60.0, description="The constant added to a rank (rrf)")
    filter_metadata: Optional[Dict[str, Any]] = Field(default=None, description="Metadata filter")


class SparseVector(BaseModel):
    """A sparse vector: term ids and their weights (BM25, SPLADE or BGE-M3 term weights)."""
    indices: List[int]
    values: List[float]


class VectorSparseQuery(BaseModel):
    """The ``k`` rows whose sparse vector (stored in the row's metadata under ``sparse_key``) has the
    greatest dot product with ``sparse``; only rows sharing a term with it are returned.  The store
    checks the limits (k at most 1024, at most 1024 terms, no repeated index); a value outside them
    is a 400."""
    user_id: str
    model_id: str
    sparse: SparseVector = Field(..., description="The query's sparse vector")
    k: int = Field(default=10, description="Rows returned")
    filter_metadata: Optional[Dict[str, Any]] = Field(default=None, description="Metadata filter")
    sparse_key: str = Field(default="sparse", description="Metadata key holding each row's sparse vector")


class VectorHybridQuery(BaseModel):
    """Dense and sparse retrieval fused by weighted reciprocal rank: the best ``fetch_k`` rows (null:
    min(200, max(k, 4 k))) for ``query`` and the best ``fetch_k`` for ``sparse`` are fused per row,
    ``weights[0] / (rrf_c + dense rank) + weights[1] / (rrf_c + sparse rank)``.  The store checks the
    limits (k and fetch_k at most 200, fetch_k >= k, two weights finite and >= 0); a value outside
    them is a 400."""
    user_id: str
    model_id: str
    query: List[float] = Field(..., description="The dense query vector")
    sparse: SparseVector = Field(..., description="The query's sparse vector")
    k: int = Field(default=10, description="Rows returned")
    fetch_k: Optional[int] = Field(default=None, description="Rows fetched per retriever")
    weights: List[float] = Field(default=[1.0, 1.0], description="(dense weight, sparse weight)")
    rrf_c: float = Field(default=60.0, description="The constant added to a rank")
    filter_metadata: Optional[Dict[str, Any]] = Field(default=None, description="Metadata filter")
    sparse_key: str = Field(default="sparse", description="Metadata key holding each row's sparse vector")


class VectorHybridSumQuery(BaseModel):
    """Dense and sparse retrieval combined by a weighted sum of the two scores: every row is ranked by
    ``weights[0] * dense + weights[1] * sparse`` (the row's exact dense key for ``query`` and the dot
    product of its sparse vector with ``sparse``, 0 for a row that shares no term), exactly over the
    whole store.  Pinecone's ``alpha`` is ``weights = [alpha, 1 - alpha]``.  The store checks the
    limits (k at most 1024, two weights in [0, 2^64]); a value outside them is a 400."""
    user_id: str
    model_id: str
    query: List[float] = Field(..., description="The dense query vector")
    sparse: SparseVector = Field(..., description="The query's sparse vector")
    k: int = Field(default=10, description="Rows returned")
    weights: List[float] = Field(default=[1.0, 1.0], description="(dense weight, sparse weight)")
    filter_metadata: Optional[Dict[str, Any]] = Field(default=None, description="Metadata filter")
    sparse_key: str = Field(default="sparse", description="Metadata key holding each row's sparse vector")


class VectorMaxSimQuery(BaseModel):
    """Late-interaction ("MaxSim") retrieval: the ``k`` best values of the metadata key ``group_by``
    (documents of a multi-vector corpus) for a set of query vectors (token embeddings).  A group's
    score is the sum, over the query vectors, of the vector's best match among the group's rows.  The
    store checks the limits (at most 64 vectors, k at most 128); a value outside them is a 400."""
    user_id: str
    model_id: str
    queries: List[List[float]] = Field(..., description="The query vectors (e.g. one per query token)")
    group_by: str = Field(..., description="Metadata key whose values are the groups (documents)")
    k: int = Field(default=10, description="Groups returned")
    filter_metadata: Optional[Dict[str, Any]] = Field(default=None, description="Metadata filter")


class VectorRecommendQuery(BaseModel):
    """Rows like the stored examples ``positive`` and unlike ``negative``: row indices, or with
    ``key`` (a metadata field, e.g. "doc_id") values of that field, every row holding one of them an
    example.  The store checks the limits (k at most 136, at most 64 examples after resolution, an
    index inside the store, a value some row holds); anything outside them is a 400."""
    user_id: str
    model_id: str
    positive: List[Union[int, str]] = Field(..., description="Examples to be like: row indices, or values of `key`")
    negative: List[Union[int, str]] = Field(default_factory=list, description="Examples to be unlike")
    k: int = Field(default=10, description="Rows returned")
    filter_metadata: Optional[Dict[str, Any]] = Field(default=None, description="Metadata filter")
    key: Optional[str] = Field(default=None, description="Metadata field the examples are values of")


class VectorRangeQuery(BaseModel):
    """Every stored row within ``threshold`` of the query: a minimum similarity for a cosine
    store, a maximum distance for a euclidean one."""
    user_id: str
    model_id: str
    query: List[float] = Field(..., description="Query vector")
    threshold: float = Field(..., description="Minimum similarity (cosine) / maximum distance (euclidean)")
    filter_metadata: Optional[Dict[str, Any]] = Field(default=None, description="Metadata filter")
    limit: int = Field(default=1000, ge=1, le=100000, description="Most results returned (the best ones)")


class VectorGroupQuery(BaseModel):
    """The ``k`` best distinct values of the metadata key ``group_by`` (the best documents of a
    chunked corpus), each with its best ``group_size`` rows."""
    user_id: str
    model_id: str
    query: List[float] = Field(..., description="Query vector")
    group_by: str = Field(..., description="Metadata key whose values are the groups")
    k: int = Field(default=10, ge=1, le=GROUP_MAX_K, description="Groups returned")
    group_size: int = Field(default=1, ge=1, le=GROUP_MAX_SIZE, description="Hits per group")
    filter_metadata: Optional[Dict[str, Any]] = Field(default=None, description="Metadata filter")


class BatchQueryRequest(BaseModel):
    user_id: str
    model_id: str
    queries: List[List[float]]
    k: int = 10
    # one filter for every query, or one entry (a filter or null) per query
    filter_metadata: Optional[Union[Dict[str, Any], List[Optional[Dict[str, Any]]]]] = None


class VectorDeleteRequest(BaseModel):
    """The body the reference's SDK sends (sdk/python/mlx_vector_db_client.py:292-303)."""
    user_id: str
    model_id: str
    filter_metadata: Dict[str, Any] = Field(..., description="Rows whose metadata matches are deleted")


class VectorDeleteResponse(BaseModel):
    success: bool
    deleted: int
    total_vectors: int
    processing_time_ms: float


class VectorUpsertRequest(VectorAddRequest):
    """/vectors/add's body plus the metadata key that names a row.  Rows are addressed by key,
    not by position: query results expose metadata only."""
    key: str = Field(default="id", description="Metadata key whose value identifies a row")


class VectorUpsertResponse(BaseModel):
    success: bool
    updated: int
    added: int
    total_vectors: int
    processing_time_ms: float


class VectorAddResponse(BaseModel):
    success: bool
    vectors_added: int
    total_vectors: int
    processing_time_ms: float


class VectorQueryResponse(BaseModel):
    results: List[Dict[str, Any]]
    query_time_ms: float
    total_vectors_searched: int


class VectorRangeQueryResponse(BaseModel):
    results: List[Dict[str, Any]]
    total_matches: int  # the exact number of rows within the threshold; may exceed len(results)
    query_time_ms: float
    total_vectors_searched: int


class VectorFusedQueryResponse(BaseModel):
    # best first: {"metadata", "fused_score", "hits", "rank"}; with fusion "max" also /vectors/query's
    # "similarity_score" and "distance" of the best-matching vector
    results: List[Dict[str, Any]]
    fusion: str
    query_time_ms: float
    total_vectors_searched: int


class VectorSparseQueryResponse(BaseModel):
    # best first: {"metadata", "sparse_score" (the dot product), "rank"}
    results: List[Dict[str, Any]]
    query_time_ms: float
    total_vectors_searched: int


class VectorHybridQueryResponse(BaseModel):
    # best first: {"metadata", "fused_score", "hits" (1 or 2: the retrievers that returned the row), "rank"}
    results: List[Dict[str, Any]]
    query_time_ms: float
    total_vectors_searched: int


class VectorHybridSumQueryResponse(BaseModel):
    # best first: {"metadata", "score" (the weighted sum), "dense_score" (the store's ranking key: the
    # cosine similarity, or minus the squared distance for euclidean), "sparse_score" (the dot product), "rank"}
    results: List[Dict[str, Any]]
    query_time_ms: float
    total_vectors_searched: int


class VectorMaxSimQueryResponse(BaseModel):
    # best group first: {"group_value", "score" (the sum in the store's ranking-key units: cosine
    # similarities, or minus the squared distances for euclidean), "rank"}
    groups: List[Dict[str, Any]]
    query_time_ms: float
    total_vectors_searched: int


class VectorGroupQueryResponse(BaseModel):
    # best group first: {"group_value": ..., "hits": [{"metadata", "similarity_score", "rank"}, ...]}
    groups: List[Dict[str, Any]]
    query_time_ms: float
    total_vectors_searched: int


class BatchQueryResponse(BaseModel):
    results: List[List[Dict[str, Any]]]
    total_queries: int
    avg_query_time_ms: float


# ---- score formatting (S12) ---------------------------------------------------------------
def format_query_results(metric: str, indices, raw_scores, metadata_list) -> List[Dict[str, Any]]:
    """/vectors/query formatting of ``store.query`` output (api/routes/vectors.py:236-258)."""
    out = []
    for i, (_idx, raw, meta) in enumerate(zip(indices, raw_scores, metadata_list)):
        similarity, distance = 0.0, 0.0
        if metric == "cosine":
            similarity = raw
            distance = 1.0 - similarity
        elif metric == "euclidean":
            distance = raw
            similarity = 1.0 / (1.0 + distance)
        elif metric == "dot_product":
            similarity = raw
            distance = -raw
        out.append({"metadata": meta, "similarity_score": similarity, "distance": distance, "rank": i + 1})
    return out


def format_batch_results(metric: str, batch_results) -> List[List[Dict[str, Any]]]:
    """/vectors/batch_query formatting of ``store.batch_query`` output (:294-317): the second
    tuple element is a distance."""
    formatted = []
    for query_results in batch_results:
        rows = []
        if isinstance(query_results, tuple) and len(query_results) == 3:
            indices, distances, metadata_list = query_results
            for i, (_idx, dist, meta) in enumerate(zip(indices, distances, metadata_list)):
                if metric == "cosine":
                    similarity = max(0, 1.0 - dist)
                elif metric == "euclidean":
                    similarity = 1.0 / (1.0 + dist)
                else:
                    similarity = max(0, -dist)
                rows.append({"metadata": meta, "similarity_score": float(similarity), "distance": float(dist),
                             "rank": i + 1})
        formatted.append(rows)
    return formatted


# ---- auth (security/auth.py:34-76): Bearer key, constant-time compare ------------------------
_bearer = HTTPBearer()
_DEFAULT_API_KEY = "mlx-vector-dev-key-2024"


def verify_api_key(credentials: HTTPAuthorizationCredentials = Security(_bearer)) -> str:
    valid = os.getenv("VECTOR_DB_API_KEY") or _DEFAULT_API_KEY
    if not credentials:
        raise HTTPException(status_code=401, detail="Authorization header required",
                            headers={"WWW-Authenticate": "Bearer"})
    if not secrets.compare_digest(credentials.credentials, valid):
        raise HTTPException(status_code=401, detail="Invalid API key", headers={"WWW-Authenticate": "Bearer"})
    return credentials.credentials


# ---- store manager (api/routes/vectors.py:37-141) --------------------------------------------
class VectorStoreManager:
    def __init__(self, config_factory: Optional[Callable[[str, str], MLXVectorStoreConfig]] = None,
                 base_dir: Optional[str] = None):
        self._stores: Dict[str, MLXVectorStore] = {}
        self._configs: Dict[str, MLXVectorStoreConfig] = {}
        self._executor = ThreadPoolExecutor(max_workers=4)
        self._lock = threading.Lock()
        self.config_factory = config_factory or (lambda user_id, model_id: MLXVectorStoreConfig())
        self.base_dir = base_dir

    def _base(self) -> Path:
        return Path(self.base_dir or os.environ.get("VECTOR_STORE_BASE", "~/.team_mind_data/vector_stores")).expanduser()

    def get_store_key(self, user_id: str, model_id: str) -> str:
        return f"{user_id}_{model_id}"

    async def get_store(self, user_id: str, model_id: str,
                        config: Optional[MLXVectorStoreConfig] = None) -> MLXVectorStore:
        key = self.get_store_key(user_id, model_id)
        if key in self._stores:
            return self._stores[key]

        def create() -> MLXVectorStore:
            with self._lock:  # one store object per key even under concurrent first requests
                if key not in self._stores:
                    cfg = config or self.config_factory(user_id, model_id)
                    self._stores[key] = MLXVectorStore(str(self._base() / user_id / model_id), cfg)
                    self._configs[key] = cfg
                    logger.info("initialised store for %s/%s", user_id, model_id)
                return self._stores[key]

        return await asyncio.get_running_loop().run_in_executor(self._executor, create)

    async def delete_store(self, user_id: str, model_id: str) -> Dict[str, Any]:
        key = self.get_store_key(user_id, model_id)
        if key not in self._stores:
            raise ValueError(f"Store not found: {user_id}/{model_id}")
        self._stores.pop(key).clear()
        self._configs.pop(key, None)
        return {"success": True, "message": f"Store {user_id}/{model_id} deleted"}

    async def warmup_all_stores(self):
        loop = asyncio.get_running_loop()
        for key, store in list(self._stores.items()):
            try:
                await loop.run_in_executor(self._executor, store._warmup_kernels)
            except Exception as e:  # the reference logs and continues (:118-119)
                logger.warning("warmup failed for %s: %s", key, e)

    def get_stats(self) -> Dict[str, Any]:
        total_vectors, total_memory = 0, 0.0
        for store in self._stores.values():
            try:
                st = store.get_stats()
                total_vectors += st.get("vector_count", 0)
                total_memory += st.get("memory_usage_mb", 0)
            except Exception as e:
                logger.warning("failed to get stats from store: %s", e)
        return {"total_stores": len(self._stores), "total_vectors": total_vectors,
                "total_memory_mb": total_memory, "mlx_optimized": True, "unified_memory": False}


def create_router(manager: Optional[VectorStoreManager] = None, auth: Callable = verify_api_key) -> APIRouter:
    """The /vectors router over `manager` (a fresh VectorStoreManager by default)."""
    mgr = manager or VectorStoreManager()
    router = APIRouter(prefix="/vectors", tags=["vectors"])
    router.store_manager = mgr  # type: ignore[attr-defined]

    @router.post("/add", response_model=VectorAddResponse)
    async def add_vectors(request: VectorAddRequest, api_key: str = Depends(auth)):
        t0 = time.time()
        try:
            store = await mgr.get_store(request.user_id, request.model_id)
            if not request.vectors or not request.metadata:
                raise HTTPException(status_code=400, detail="Vectors and metadata required")
            import numpy as np
            vectors_np = np.array(request.vectors, dtype=np.float32)
            loop = asyncio.get_running_loop()
            await loop.run_in_executor(mgr._executor, lambda: store.add_vectors(vectors_np, request.metadata))
            return VectorAddResponse(success=True, vectors_added=len(request.vectors),
                                     total_vectors=store.get_stats().get("vector_count", 0),
                                     processing_time_ms=(time.time() - t0) * 1000)
        except Exception as e:  # the reference turns every error, its own 400s included, into a 500
            logger.error("Error adding vectors: %s", e)
            raise HTTPException(status_code=500, detail=f"Failed to add vectors: {e}")

    @router.post("/query", response_model=VectorQueryResponse)
    async def query_vectors(request: VectorQuery, api_key: str = Depends(auth)):
        t0 = time.time()
        try:
            store = await mgr.get_store(request.user_id, request.model_id)
            if not request.query:
                raise HTTPException(status_code=400, detail="Query vector required")
            loop = asyncio.get_running_loop()
            indices, scores, metas = await loop.run_in_executor(
                mgr._executor, lambda: store.query(request.query, k=request.k,
                                                   filter_metadata=request.filter_metadata))
            return VectorQueryResponse(results=format_query_results(store.config.metric, indices, scores, metas),
                                       query_time_ms=(time.time() - t0) * 1000,
                                       total_vectors_searched=store.get_stats().get("vector_count", 0))
        except FilterError as e:  # a malformed filter condition is the caller's error (nothing the reference has)
            raise HTTPException(status_code=400, detail=f"Query failed: {e}")
        except Exception as e:  # the reference turns every error, its own 400s included, into a 500
            logger.error("Error querying vectors: %s", e, exc_info=True)
            raise HTTPException(status_code=500, detail=f"Query failed: {e}")

    @router.post("/range_query", response_model=VectorRangeQueryResponse)
    async def range_query_vectors(request: VectorRangeQuery, api_key: str = Depends(auth)):
        """Every row within the threshold, best first, at most ``limit`` of them; ``total_matches``
        is the exact count.  A bad request (empty query, NaN threshold, negative radius, dimension
        mismatch: the store's ValueError) is a 400, an unsupported store a 501, anything else a 500."""
        t0 = time.time()
        try:
            store = await mgr.get_store(request.user_id, request.model_id)
            if not request.query:
                raise HTTPException(status_code=400, detail="Query vector required")

            # the best `limit` hits and the exact total from one device call: no more than `limit`
            # result entries are ever built
            loop = asyncio.get_running_loop()
            indices, scores, metas, total = await loop.run_in_executor(
                mgr._executor, lambda: store.range_query(request.query, request.threshold,
                                                         filter_metadata=request.filter_metadata,
                                                         limit=request.limit, with_total=True))
            return VectorRangeQueryResponse(results=format_query_results(store.config.metric, indices, scores, metas),
                                            total_matches=total, query_time_ms=(time.time() - t0) * 1000,
                                            total_vectors_searched=store.get_stats().get("vector_count", 0))
        except HTTPException:
            raise
        except ValueError as e:
            raise HTTPException(status_code=400, detail=f"Range query failed: {e}")
        except NotImplementedError as e:
            raise HTTPException(status_code=501, detail=f"Range query failed: {e}")
        except Exception as e:
            logger.error("Error in range query: %s", e, exc_info=True)
            raise HTTPException(status_code=500, detail=f"Range query failed: {e}")

    @router.post("/query_groups", response_model=VectorGroupQueryResponse)
    async def query_groups_vectors(request: VectorGroupQuery, api_key: str = Depends(auth)):
        """The ``k`` best groups (distinct values of ``group_by``), best first, each with its best
        ``group_size`` hits.  A bad request (empty query, dimension mismatch: the store's
        ValueError) is a 400, an unsupported store a 501, anything else a 500."""
        t0 = time.time()
        try:
            store = await mgr.get_store(request.user_id, request.model_id)
            if not request.query:
                raise HTTPException(status_code=400, detail="Query vector required")
            loop = asyncio.get_running_loop()
            groups = await loop.run_in_executor(
                mgr._executor, lambda: store.query_groups(request.query, request.group_by, k=request.k,
                                                          group_size=request.group_size,
                                                          filter_metadata=request.filter_metadata))
            out = [{"group_value": g["group"], "hits": format_query_results(store.config.metric, *g["hits"])}
                   for g in groups]
            return VectorGroupQueryResponse(groups=out, query_time_ms=(time.time() - t0) * 1000,
                                            total_vectors_searched=store.get_stats().get("vector_count", 0))
        except HTTPException:
            raise
        except ValueError as e:
            raise HTTPException(status_code=400, detail=f"Grouped query failed: {e}")
        except NotImplementedError as e:
            raise HTTPException(status_code=501, detail=f"Grouped query failed: {e}")
        except Exception as e:
            logger.error("Error in grouped query: %s", e, exc_info=True)
            raise HTTPException(status_code=500, detail=f"Grouped query failed: {e}")

    @router.post("/mmr_query", response_model=VectorQueryResponse)
    async def mmr_query_vectors(request: VectorMMRQuery, api_key: str = Depends(auth)):
        """``k`` relevant and mutually diverse rows (maximal marginal relevance) in pick order, in
        /vectors/query's format.  A bad request (empty query, k / fetch_k / lambda_mult outside their
        limits, dimension mismatch: the store's ValueError) is a 400, an unsupported store a 501,
        anything else a 500."""
        t0 = time.time()
        try:
            store = await mgr.get_store(request.user_id, request.model_id)
            if not request.query:
                raise HTTPException(status_code=400, detail="Query vector required")
            loop = asyncio.get_running_loop()
            indices, scores, metas = await loop.run_in_executor(
                mgr._executor, lambda: store.mmr_query(request.query, k=request.k, fetch_k=request.fetch_k,
                                                       lambda_mult=request.lambda_mult,
                                                       filter_metadata=request.filter_metadata))
            return VectorQueryResponse(results=format_query_results(store.config.metric, indices, scores, metas),
                                       query_time_ms=(time.time() - t0) * 1000,
                                       total_vectors_searched=store.get_stats().get("vector_count", 0))
        except HTTPException:
            raise
        except ValueError as e:
            raise HTTPException(status_code=400, detail=f"MMR query failed: {e}")
        except NotImplementedError as e:
            raise HTTPException(status_code=501, detail=f"MMR query failed: {e}")
        except Exception as e:
            logger.error("Error in MMR query: %s", e, exc_info=True)
            raise HTTPException(status_code=500, detail=f"MMR query failed: {e}")

    @router.post("/fused_query", response_model=VectorFusedQueryResponse)
    async def fused_query_vectors(request: VectorFusedQuery, api_key: str = Depends(auth)):
        """One ranked list from several query vectors, fused by weighted reciprocal rank or by the
        best match to any of them.  A bad request (no vector, more than 16, k / fetch_k / rrf_c /
        weights outside their limits, an unknown fusion, dimension mismatch: the store's ValueError)
        is a 400, an unsupported store a 501, anything else a 500."""
        t0 = time.time()
        try:
            store = await mgr.get_store(request.user_id, request.model_id)
            if not request.queries or not all(request.queries):
                raise HTTPException(status_code=400, detail="Query vectors required")
            loop = asyncio.get_running_loop()
            indices, scores, metas, fused, hits = await loop.run_in_executor(
                mgr._executor, lambda: store.fused_query(request.queries, k=request.k, fusion=request.fusion,
                                                         weights=request.weights, fetch_k=request.fetch_k,
                                                         rrf_c=request.rrf_c, filter_metadata=request.filter_metadata))
            if request.fusion == "max":
                results = format_query_results(store.config.metric, indices, scores, metas)
            else:
                results = [{"metadata": m, "rank": i + 1} for i, m in enumerate(metas)]
            for r, f, h in zip(results, fused, hits):
                r["fused_score"] = f
                r["hits"] = h
            return VectorFusedQueryResponse(results=results, fusion=request.fusion,
                                            query_time_ms=(time.time() - t0) * 1000,
                                            total_vectors_searched=store.get_stats().get("vector_count", 0))
        except HTTPException:
            raise
        except ValueError as e:
            raise HTTPException(status_code=400, detail=f"Fused query failed: {e}")
        except NotImplementedError as e:
            raise HTTPException(status_code=501, detail=f"Fused query failed: {e}")
        except Exception as e:
            logger.error("Error in fused query: %s", e, exc_info=True)
            raise HTTPException(status_code=500, detail=f"Fused query failed: {e}")

    @router.post("/sparse_query", response_model=VectorSparseQueryResponse)
    async def sparse_query_vectors(request: VectorSparseQuery, api_key: str = Depends(auth)):
        """The ``k`` rows with the greatest sparse dot product, best first.  A bad request (k outside
        its limits, a repeated index, too many terms: the store's ValueError) is a 400, an
        unsupported store a 501, anything else a 500."""
        t0 = time.time()
        try:
            store = await mgr.get_store(request.user_id, request.model_id)
            sparse = {"indices": request.sparse.indices, "values": request.sparse.values}
            loop = asyncio.get_running_loop()
            indices, scores, metas = await loop.run_in_executor(
                mgr._executor, lambda: store.sparse_query(sparse, k=request.k, filter_metadata=request.filter_metadata,
                                                          sparse_key=request.sparse_key))
            results = [{"metadata": m, "sparse_score": s, "rank": i + 1} for i, (m, s) in enumerate(zip(metas, scores))]
            return VectorSparseQueryResponse(results=results, query_time_ms=(time.time() - t0) * 1000,
                                             total_vectors_searched=store.get_stats().get("vector_count", 0))
        except HTTPException:
            raise
        except ValueError as e:
            raise HTTPException(status_code=400, detail=f"Sparse query failed: {e}")
        except NotImplementedError as e:
            raise HTTPException(status_code=501, detail=f"Sparse query failed: {e}")
        except Exception as e:
            logger.error("Error in sparse query: %s", e, exc_info=True)
            raise HTTPException(status_code=500, detail=f"Sparse query failed: {e}")

    @router.post("/hybrid_query", response_model=VectorHybridQueryResponse)
    async def hybrid_query_vectors(request: VectorHybridQuery, api_key: str = Depends(auth)):
        """Dense and sparse retrieval fused by weighted reciprocal rank, best first.  A bad request
        (no vector, k / fetch_k / rrf_c / weights outside their limits, a bad sparse vector, dimension
        mismatch: the store's ValueError) is a 400, an unsupported store a 501, anything else a 500."""
        t0 = time.time()
        try:
            store = await mgr.get_store(request.user_id, request.model_id)
            if not request.query:
                raise HTTPException(status_code=400, detail="Query vector required")
            sparse = {"indices": request.sparse.indices, "values": request.sparse.values}
            loop = asyncio.get_running_loop()
            indices, scores, metas, fused, hits = await loop.run_in_executor(
                mgr._executor, lambda: store.hybrid_query(request.query, sparse, k=request.k, fetch_k=request.fetch_k,
                                                          weights=request.weights, rrf_c=request.rrf_c,
                                                          filter_metadata=request.filter_metadata,
                                                          sparse_key=request.sparse_key))
            results = [{"metadata": m, "fused_score": f, "hits": h, "rank": i + 1}
                       for i, (m, f, h) in enumerate(zip(metas, fused, hits))]
            return VectorHybridQueryResponse(results=results, query_time_ms=(time.time() - t0) * 1000,
                                             total_vectors_searched=store.get_stats().get("vector_count", 0))
        except HTTPException:
            raise
        except ValueError as e:
            raise HTTPException(status_code=400, detail=f"Hybrid query failed: {e}")
        except NotImplementedError as e:
            raise HTTPException(status_code=501, detail=f"Hybrid query failed: {e}")
        except Exception as e:
            logger.error("Error in hybrid query: %s", e, exc_info=True)
            raise HTTPException(status_code=500, detail=f"Hybrid query failed: {e}")

    @router.post("/hybrid_sum_query", response_model=VectorHybridSumQueryResponse)
    async def hybrid_sum_query_vectors(request: VectorHybridSumQuery, api_key: str = Depends(auth)):
        """Dense and sparse retrieval combined by a weighted sum of the two scores, best first.  A bad
        request (no vector, k / weights outside their limits, a bad sparse vector, dimension mismatch:
        the store's ValueError) is a 400, an unsupported store a 501, anything else a 500."""
        t0 = time.time()
        try:
            store = await mgr.get_store(request.user_id, request.model_id)
            if not request.query:
                raise HTTPException(status_code=400, detail="Query vector required")
            sparse = {"indices": request.sparse.indices, "values": request.sparse.values}
            loop = asyncio.get_running_loop()
            indices, scores, metas, dense, sparse_scores = await loop.run_in_executor(
                mgr._executor, lambda: store.hybrid_sum_query(request.query, sparse, k=request.k, weights=request.weights,
                                                              filter_metadata=request.filter_metadata,
                                                              sparse_key=request.sparse_key))
            results = [{"metadata": m, "score": c, "dense_score": d, "sparse_score": p, "rank": i + 1}
                       for i, (m, c, d, p) in enumerate(zip(metas, scores, dense, sparse_scores))]
            return VectorHybridSumQueryResponse(results=results, query_time_ms=(time.time() - t0) * 1000,
                                                total_vectors_searched=store.get_stats().get("vector_count", 0))
        except HTTPException:
            raise
        except ValueError as e:
            raise HTTPException(status_code=400, detail=f"Hybrid sum query failed: {e}")
        except NotImplementedError as e:
            raise HTTPException(status_code=501, detail=f"Hybrid sum query failed: {e}")
        except Exception as e:
            logger.error("Error in hybrid sum query: %s", e, exc_info=True)
            raise HTTPException(status_code=500, detail=f"Hybrid sum query failed: {e}")

    @router.post("/maxsim_query", response_model=VectorMaxSimQueryResponse)
    async def maxsim_query_vectors(request: VectorMaxSimQuery, api_key: str = Depends(auth)):
        """The ``k`` best groups (distinct values of ``group_by``) by the summed best match of every
        query vector, best first.  A bad request (no vector, more than 64, k outside its limits,
        dimension mismatch: the store's ValueError) is a 400, an unsupported store a 501, anything
        else a 500."""
        t0 = time.time()
        try:
            store = await mgr.get_store(request.user_id, request.model_id)
            if not request.queries or not all(request.queries):
                raise HTTPException(status_code=400, detail="Query vectors required")
            loop = asyncio.get_running_loop()
            groups = await loop.run_in_executor(
                mgr._executor, lambda: store.maxsim_query(request.queries, request.group_by, k=request.k,
                                                          filter_metadata=request.filter_metadata))
            out = [{"group_value": g["group"], "score": g["sum"], "rank": i + 1} for i, g in enumerate(groups)]
            return VectorMaxSimQueryResponse(groups=out, query_time_ms=(time.time() - t0) * 1000,
                                             total_vectors_searched=store.get_stats().get("vector_count", 0))
        except HTTPException:
            raise
        except ValueError as e:
            raise HTTPException(status_code=400, detail=f"MaxSim query failed: {e}")
        except NotImplementedError as e:
            raise HTTPException(status_code=501, detail=f"MaxSim query failed: {e}")
        except Exception as e:
            logger.error("Error in MaxSim query: %s", e, exc_info=True)
            raise HTTPException(status_code=500, detail=f"MaxSim query failed: {e}")

    @router.post("/recommend", response_model=VectorQueryResponse)
    async def recommend_vectors(request: VectorRecommendQuery, api_key: str = Depends(auth)):
        """The ``k`` rows most like the stored examples ``positive`` and unlike ``negative``, the
        examples left out, in /vectors/query's format.  A bad request (k or the example count
        outside their limits, an index outside the store, a ``key`` value no row holds: the store's
        ValueError) is a 400, an unsupported store a 501, anything else a 500."""
        t0 = time.time()
        try:
            store = await mgr.get_store(request.user_id, request.model_id)
            loop = asyncio.get_running_loop()
            indices, scores, metas = await loop.run_in_executor(
                mgr._executor, lambda: store.recommend(request.positive, request.negative, k=request.k,
                                                       filter_metadata=request.filter_metadata, key=request.key))
            return VectorQueryResponse(results=format_query_results(store.config.metric, indices, scores, metas),
                                       query_time_ms=(time.time() - t0) * 1000,
                                       total_vectors_searched=store.get_stats().get("vector_count", 0))
        except HTTPException:
            raise
        except ValueError as e:
            raise HTTPException(status_code=400, detail=f"Recommend failed: {e}")
        except NotImplementedError as e:
            raise HTTPException(status_code=501, detail=f"Recommend failed: {e}")
        except Exception as e:
            logger.error("Error in recommend: %s", e, exc_info=True)
            raise HTTPException(status_code=500, detail=f"Recommend failed: {e}")

    @router.post("/batch_query", response_model=BatchQueryResponse)
    async def batch_query_vectors(request: BatchQueryRequest, api_key: str = Depends(auth)):
        t0 = time.time()
        try:
            store = await mgr.get_store(request.user_id, request.model_id)
            if not request.queries:
                raise HTTPException(status_code=400, detail="Query vectors required")
            filt = request.filter_metadata
            if isinstance(filt, list) and len(filt) != len(request.queries):
                raise HTTPException(status_code=400,
                                    detail=f"{len(request.queries)} queries but {len(filt)} filters")
            kw = {} if filt is None else {"filter_metadata": filt}  # (without one: the call as it always was)
            loop = asyncio.get_running_loop()
            batch = await loop.run_in_executor(mgr._executor,
                                               lambda: store.batch_query(request.queries, k=request.k, **kw))
            total = (time.time() - t0) * 1000
            return BatchQueryResponse(results=format_batch_results(store.config.metric, batch),
                                      total_queries=len(request.queries),
                                      avg_query_time_ms=total / len(request.queries))
        except FilterError as e:  # as /query: a malformed filter condition is a 400
            raise HTTPException(status_code=400, detail=f"Batch query failed: {e}")
        except Exception as e:  # the reference turns every error, its own 400s included, into a 500
            logger.error("Error in batch query: %s", e)
            raise HTTPException(status_code=500, detail=f"Batch query failed: {e}")

    @router.post("/delete", response_model=VectorDeleteResponse)
    async def delete_vectors(request: VectorDeleteRequest, api_key: str = Depends(auth)):
        t0 = time.time()
        try:
            store = await mgr.get_store(request.user_id, request.model_id)
            loop = asyncio.get_running_loop()
            res = await loop.run_in_executor(mgr._executor,
                                             lambda: store.delete_vectors(request.filter_metadata))
            return VectorDeleteResponse(success=True, deleted=res["deleted"], total_vectors=res["total_vectors"],
                                        processing_time_ms=(time.time() - t0) * 1000)
        except FilterError as e:  # as /query: a malformed filter condition is a 400
            raise HTTPException(status_code=400, detail=f"Failed to delete vectors: {e}")
        except Exception as e:  # as the sibling routes: every other error becomes a 500
            logger.error("Error deleting vectors: %s", e)
            raise HTTPException(status_code=500, detail=f"Failed to delete vectors: {e}")

    @router.post("/upsert", response_model=VectorUpsertResponse)
    async def upsert_vectors(request: VectorUpsertRequest, api_key: str = Depends(auth)):
        t0 = time.time()
        try:
            store = await mgr.get_store(request.user_id, request.model_id)
            if not request.vectors or not request.metadata:
                raise HTTPException(status_code=400, detail="Vectors and metadata required")
            import numpy as np
            vectors_np = np.array(request.vectors, dtype=np.float32)
            loop = asyncio.get_running_loop()
            res = await loop.run_in_executor(
                mgr._executor, lambda: store.upsert_vectors(vectors_np, request.metadata, key=request.key))
            return VectorUpsertResponse(success=True, updated=res["updated"], added=res["added"],
                                        total_vectors=res["total_vectors"],
                                        processing_time_ms=(time.time() - t0) * 1000)
        except Exception as e:  # as /vectors/add: every error, a store ValueError included, becomes a 500
            logger.error("Error upserting vectors: %s", e)
            raise HTTPException(status_code=500, detail=f"Failed to upsert vectors: {e}")

    @router.get("/count")
    async def get_vector_count(user_id: str, model_id: str, api_key: str = Depends(auth)):
        try:
            store = await mgr.get_store(user_id, model_id)
            return {"count": store.get_stats().get("vector_count", 0)}
        except Exception as e:
            raise HTTPException(status_code=500, detail=str(e))

    @router.get("/stats")
    async def get_store_stats(user_id: str, model_id: str, api_key: str = Depends(auth)):
        try:
            store = await mgr.get_store(user_id, model_id)
            return {"store_stats": store.get_stats(),
                    "performance_info": {"mlx_optimized": True, "expected_qps": "800-1500",
                                         "target_latency": "<10ms"}}
        except Exception as e:
            raise HTTPException(status_code=500, detail=str(e))

    @router.get("/health")
    async def health_check():
        try:
            g = mgr.get_stats()
            return {"status": "healthy", "mlx_optimized": True, "stores_active": g["total_stores"],
                    "total_vectors": g["total_vectors"], "memory_usage_mb": g["total_memory_mb"]}
        except Exception as e:
            return {"status": "unhealthy", "error": str(e)}

    return router


def create_app(manager: Optional[VectorStoreManager] = None, auth: Callable = verify_api_key):
    """A FastAPI app serving only the /vectors routes (main.py:205 mounts the same router)."""
    from fastapi import FastAPI
    app = FastAPI(title="MLX Vector DB (MI355X core)")
    app.include_router(create_router(manager, auth))
    return app


# module-level router like the reference's (main.py imports `router` from this module)
store_manager = VectorStoreManager()
router = create_router(store_manager)
