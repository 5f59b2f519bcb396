"""Drop-in store for the brute-force hot path, backed by the gfx950 vdb core.

Mirrors the reference module ``service/optimized_vector_store.py`` (same class
and function names, argument meaning, return shapes and error behaviour) so
that existing callers — the REST routes (api/routes/vectors.py:57-64, :193,
:229-233, :291), the admin routes, the RAG pipeline and the benchmarks — run
unchanged with ``mlx-vector-db_amd/`` first on ``sys.path``.

What differs underneath:
  * the corpus lives on the GPU as row-major fp32 rows plus an int8 copy of the
    centred rows (two planes in MFMA operand tiles; a split-bf16 copy is built
    only if a search needs one), with norms computed once at ingest (the
    reference re-normalises every row on every query,
    service/optimized_vector_store.py:31-41);
  * search is a fused int8-MFMA candidate pass (I8 for k <= 16, I8X3 above;
    uncertified queries re-passed or sent to the exact scan) + exact fp64 rerank
    and certificate instead of a full argsort (:176-183); ranking is exact with
    ties to the lower row;
  * ``batch_query``, ``optimize`` and ``health_check`` exist (callers expect
    them: api/routes/vectors.py:291, api/routes/admin.py:230, tests/demo.py:134,
    :248, :254) and the functional API of tests/test_vector_store.py:15-18.
"""
from __future__ import annotations

import json
import logging
import os
import collections
from collections import OrderedDict
import shutil
import threading
import time
from dataclasses import dataclass
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np

from . import _vdb, filter_ops
from .metadata_index import MetadataIndex
from .persistence import StoreFiles

logger = logging.getLogger("mlx_vector_db.optimized_store")

# Raised by the reference when no similarity operator exists (jit_compile=False
# or metric="dot_product"): service/optimized_vector_store.py:153-154.
_NO_OPERATOR_MSG = "Keine kompilierte Ähnlichkeitsfunktion verfügbar."
# query_groups: the most groups per query (include/vdb.h vdb_index_search_groups) and the most hits
# per group; POST /vectors/query_groups bounds its body by the same two
GROUP_MAX_K = 128
GROUP_MAX_SIZE = 100
# mmr_query: the most rows per query and the most candidates they are picked from (include/vdb.h
# vdb_index_search_mmr); POST /vectors/mmr_query answers a value outside them with 400
MMR_MAX_K = 200
MMR_MAX_FETCH = 200
# recommend: the most rows per query and the most examples (positives and negatives together) a
# query is built from (include/vdb.h vdb_index_search_recommend); POST /vectors/recommend answers a
# value outside them with 400
REC_MAX_K = 136
REC_MAX_EXAMPLES = 64
# fused_query: the most rows per set, the most rows fetched per vector and the most vectors per set
# (include/vdb.h vdb_index_search_fused); POST /vectors/fused_query answers a value outside them with
# 400
FUSED_MAX_K = 200
FUSED_MAX_FETCH = 200
FUSED_MAX_LISTS = 16
# maxsim_query: the most groups per set, the most vectors per set and the most table entries (query
# vectors of a call x distinct group values) of one device call (include/vdb.h
# vdb_index_search_maxsim); POST /vectors/maxsim_query answers a value outside them with 400
MAXSIM_MAX_K = 128
MAXSIM_MAX_VECTORS = 64
MAXSIM_MAX_CELLS = 1 << 27
# sparse_query / hybrid_query: the most rows per sparse query and the most terms a query's sparse
# vector may hold (include/vdb.h vdb_index_search_sparse; hybrid_query's k and fetch_k follow
# FUSED_MAX_*); POST /vectors/sparse_query and /vectors/hybrid_query answer a value outside them with 400
SPARSE_MAX_K = 1024
SPARSE_MAX_QUERY_TERMS = 1024
# hybrid_sum_query: the most rows per query, the most queries of one call and the greatest weight
# (include/vdb.h vdb_index_search_hybrid_sum); POST /vectors/hybrid_sum_query answers a value outside
# them with 400
HYBRID_SUM_MAX_K = _vdb.HYBRID_SUM_MAX_K
HYBRID_SUM_MAX_QUERIES = 65535
HYBRID_SUM_MAX_WEIGHT = 2.0 ** 64


def _sparse_pair(value, what: str):
    """``{"indices": [...], "values": [...]}`` -> (int64 indices, fp32 values) sorted by index; a
    repeated index, a negative or non-integer one, lengths that differ or a non-finite value raise
    ValueError."""
    if not isinstance(value, dict) or "indices" not in value or "values" not in value:
        raise ValueError(f'{what} must be {{"indices": [...], "values": [...]}}')
    idx = np.asarray(value["indices"])
    if idx.size and idx.dtype.kind not in "iu":
        raise ValueError(f"{what}: indices must be integers")
    idx = idx.astype(np.int64, copy=False).reshape(-1)
    val = np.asarray(value["values"], dtype=np.float64).reshape(-1)
    if idx.size != val.size:
        raise ValueError(f"{what}: {idx.size} indices but {val.size} values")
    if idx.size and (int(idx.min()) < 0 or int(idx.max()) > 2**31 - 2):
        raise ValueError(f"{what}: indices must be in [0, 2^31 - 2]")
    if not (np.isfinite(val).all() and (np.abs(val) <= float(np.finfo(np.float32).max)).all()):
        raise ValueError(f"{what}: values must be finite in fp32")
    order = np.argsort(idx, kind="stable")
    idx, val = idx[order], val[order]
    if idx.size > 1 and (np.diff(idx) == 0).any():
        raise ValueError(f"{what}: index {int(idx[1:][np.diff(idx) == 0][0])} is repeated")
    return idx, val.astype(np.float32)


def build_sparse_column(metadata: List[Dict], n: int, sparse_key: str = "sparse"):
    """The CSR column ``vdb_index_set_sparse`` takes, from the first ``n`` rows' metadata: row r's
    sparse vector is ``metadata[r][sparse_key]`` (``{"indices": [...], "values": [...]}``, sorted
    here; a repeated index is a ValueError), a row without the key has no entry.  -> (indptr int64
    [n + 1], terms int32, weights fp32, n_terms); n_terms is one more than the largest index seen, 0
    when no row has an entry."""
    ts, ws = [], []
    indptr = np.zeros(n + 1, np.int64)
    for r in range(n):
        m = metadata[r] if r < len(metadata) else None
        v = m.get(sparse_key) if isinstance(m, dict) else None
        if v is not None:
            t, w = _sparse_pair(v, f"row {r}: metadata[{sparse_key!r}]")
            ts.append(t)
            ws.append(w)
            indptr[r + 1] = t.size
    np.cumsum(indptr, out=indptr)
    terms = np.concatenate(ts).astype(np.int32) if ts else np.zeros(0, np.int32)
    weights = np.concatenate(ws).astype(np.float32) if ws else np.zeros(0, np.float32)
    n_terms = int(terms.max()) + 1 if terms.size else 0
    return indptr, terms, weights, n_terms


def normalize_sparse_query(sparse):
    """A query's sparse vector (``{"indices", "values"}``, or None for none) -> (indices, values)
    sorted by index with the zero weights dropped; a repeated index or more than
    SPARSE_MAX_QUERY_TERMS terms is a ValueError."""
    if sparse is None:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    idx, val = _sparse_pair(sparse, "the query's sparse vector")
    keep = val != 0
    idx, val = idx[keep], val[keep]
    if idx.size > SPARSE_MAX_QUERY_TERMS:
        raise ValueError(f"a query's sparse vector takes at most {SPARSE_MAX_QUERY_TERMS} terms, got {idx.size}")
    return idx, val


def clip_sparse_query(q, n_terms: int):
    """A normalised query without the indices at or past ``n_terms``: no row can hold them."""
    idx, val = q
    keep = idx < n_terms
    return idx[keep].astype(np.int32), val[keep]


# half the smallest measured crossover of the row-list search against the masked
# search (0.0136 % of the rows: 1 M x 128 L2, 64 queries sharing one list)
SUBSET_MAX_FRACTION_DEFAULT = 6.8e-5


@dataclass
class MLXVectorStoreConfig:
    """service/optimized_vector_store.py:51-56, plus two MI355X knobs."""
    dimension: int = 384
    metric: str = "cosine"
    enable_hnsw: bool = False
    jit_compile: bool = True
    device: int = 0          # GPU ordinal holding this store's corpus
    persist: bool = True     # persist every add (append log + periodic compaction, service/persistence.py)
    # several GPUs of this process: the corpus is row-sharded over them, each query batch is
    # searched on every shard at once and the per-shard top-k lists are gathered and merged
    # on the first device (service/_vdb.py NativeShards); None = the single `device`
    devices: Optional[List[int]] = None
    # concurrent single-vector queries (the REST executor's 4 threads, api/routes/vectors.py:43)
    # join one batched device search instead of one corpus scan each (_QueryCoalescer)
    coalesce: bool = True
    coalesce_inflight: int = 2  # coalesced batches running at once (each on its own stream)
    # a batch leader's wait for the rest of a wave of callers (C2, 4 threads, 2 in flight: 8.6-8.9 K
    # QPS at 300 us against 8.3 K without, profiles/r06_serve/serving.txt; a lone caller never waits)
    coalesce_linger_us: float = 300.0
    # a filter whose eligible rows are at most this fraction of the store is searched as an explicit
    # row list (include/vdb.h vdb_index_search_rows: only those rows are read, and queries with
    # different filters share one call, so they coalesce too); above it, or on a multi-device store,
    # as a row_mask over the whole corpus.  0 disables the row-list path.  Results are identical
    # either way; the value is half the smaller measured crossover.
    subset_max_fraction: float = SUBSET_MAX_FRACTION_DEFAULT


def _filter_key(filt: Dict):
    """Grouping key of a filter: equal for filters holding the same pairs and conditions (as the
    bitmap cache keys them; a condition dict is canonicalised into a tuple, so equal conditions
    written as separate dict objects share a group); a filter with an unhashable value is its own
    group."""
    try:
        return filter_ops.canonical_key(filt)
    except TypeError:
        return ("unhashable", id(filt))


def _mask_rows(mask: np.ndarray, n: int) -> np.ndarray:
    """The rows < n a uint32 bitmap marks, ascending (int64): the row list of a mask the device
    built.  Only the non-zero words are unpacked: a pass over n / 32 words, then work per set word,
    not per row (a row list is taken for filters that match a few rows of many)."""
    words = np.ascontiguousarray(mask, np.uint32).reshape(-1)[:(n + 31) // 32]
    nz = np.nonzero(words)[0]
    if nz.size == 0:
        return np.zeros(0, np.int64)
    bits = np.unpackbits(words[nz].astype("<u4").view(np.uint8).reshape(-1, 4), axis=1, bitorder="little")
    w, b = np.nonzero(bits)
    rows = nz[w].astype(np.int64) * 32 + b
    return rows[rows < n]


def _as_matrix(vectors: Any) -> np.ndarray:
    """mx.array(vectors, float32) restated (service/optimized_vector_store.py:215-216)."""
    if hasattr(vectors, "detach") and hasattr(vectors, "cpu"):  # torch tensor
        vectors = vectors.detach().cpu().numpy()
    a = np.asarray(vectors, dtype=np.float32)
    return a


class _RWLock:
    """Many readers (queries) or one writer (add / clear / optimize).  The reference
    takes an RLock in add_vectors and clear but none in query
    (service/optimized_vector_store.py:97,116,199) and is served from a 4-thread
    executor (api/routes/vectors.py:43); here queries still run concurrently with each
    other (ctypes releases the GIL inside the C-ABI), but always see a consistent
    (rows, metadata) snapshot instead of a half-applied add."""

    def __init__(self):
        self._cond = threading.Condition(threading.Lock())
        self._readers = 0
        self._writer = False
        self._waiting_writers = 0

    def acquire_read(self):
        with self._cond:
            while self._writer or self._waiting_writers:
                self._cond.wait()
            self._readers += 1

    def release_read(self):
        with self._cond:
            self._readers -= 1
            if self._readers == 0:
                self._cond.notify_all()

    def acquire_write(self):
        with self._cond:
            self._waiting_writers += 1
            while self._writer or self._readers:
                self._cond.wait()
            self._waiting_writers -= 1
            self._writer = True

    def release_write(self):
        with self._cond:
            self._writer = False
            self._cond.notify_all()


class _Read:
    def __init__(self, lk: _RWLock):
        self.lk = lk

    def __enter__(self):
        self.lk.acquire_read()

    def __exit__(self, *a):
        self.lk.release_read()


class _Write(_Read):
    def __enter__(self):
        self.lk.acquire_write()

    def __exit__(self, *a):
        self.lk.release_write()


class _QueryCoalescer:
    """Continuous batching of concurrent single-vector queries, pipelined.

    The reference serves /vectors/query one vector per request from a 4-thread executor
    (api/routes/vectors.py:43, :226-234): each call is a full scan of the corpus
    (service/optimized_vector_store.py:149-192).  A scan costs about the same for 1 query as
    for 64 (the corpus read dominates), so the queries that arrive while batches
    run wait and then run together as the next batch: no artificial delay when a query arrives
    alone, up to ``max_batch`` queries per scan under load.  Up to ``max_inflight`` batches
    run at once (each on its own workspace stream of the index, so one batch's host work and
    tail kernels overlap another's scan; with one batch in flight the device idled during the
    host side and 4 direct callers beat the coalescer).  A batch holds requests of
    one k class (k <= 16 / <= 200 / larger: the candidate pass a batch runs depends on its
    largest k, so one caller's large k does not move its co-batched callers to a slower pass);
    each caller gets its own row and k (the exact order makes every caller's top-k the prefix
    of the batch's).  A batch also holds either only unfiltered requests (``run(Q, k)``) or only
    filtered ones whose filters the store searches as row lists (``run(Q, k, filters)``, one
    filter per query in order: one device call whatever the filters are).  Callers hold the store's
    read lock while they wait, so every query of a batch sees the same rows."""

    def __init__(self, run, max_batch: int = 64, max_inflight: int = 2, linger_us: float = 0.0):
        # run(Q [B, D], k) -> [(indices, scores, metadata)] * B; filtered batches: run(Q, k, filters)
        self._run = run
        self._max = max_batch
        self._inflight = max(1, int(max_inflight))
        # adaptive linger: callers come back in waves (each waits for its own result), so a leader
        # that finds fewer pending queries than the recent batches held waits up to linger_us for
        # the rest of the wave; a lone caller (recent batches of 1) never waits
        self._linger = max(0.0, float(linger_us)) * 1e-6
        self._recent = collections.deque(maxlen=8)
        self._cv = threading.Condition(threading.Lock())
        self._pending: List[list] = []
        self._running = 0
        self.batches = 0
        self.queries = 0

    @staticmethod
    def _kclass(k: int) -> int:
        return 0 if k <= 16 else 1 if k <= 200 else 2

    def query(self, q: np.ndarray, k: int, filt=None):
        req = [q, int(k), None, None, filt]  # query, k, result, error, filter (None: unfiltered)
        self._cv.acquire()
        try:
            self._pending.append(req)
            # wait for a result; whenever fewer than max_inflight batches run, lead the next one:
            # the oldest pending request's k class, FIFO (a leader may serve others before its own)
            lingered = False
            while req[2] is None and req[3] is None:
                if self._running >= self._inflight or not self._pending:
                    self._cv.wait()
                    continue
                expect = min(self._max, max(self._recent)) if self._recent else 1
                if self._linger > 0.0 and not lingered and len(self._pending) < expect:
                    lingered = True
                    deadline = time.perf_counter() + self._linger
                    while len(self._pending) < expect and req[2] is None and req[3] is None:
                        rem = deadline - time.perf_counter()
                        if rem <= 0.0:
                            break
                        self._cv.wait(rem)
                    continue  # (another leader may have taken the requests meanwhile)
                kc = self._kclass(self._pending[0][1])
                fk = self._pending[0][4] is not None  # ... and its kind: filtered or not
                batch, rest = [], []
                for r in self._pending:
                    (batch if len(batch) < self._max and self._kclass(r[1]) == kc and (r[4] is not None) == fk
                     else rest).append(r)
                self._pending = rest
                self._running += 1
                self._cv.release()
                try:
                    kmax = max(r[1] for r in batch)
                    Q = np.stack([r[0] for r in batch])
                    res = self._run(Q, kmax, [r[4] for r in batch]) if fk else self._run(Q, kmax)
                    for r, (ix, sc, md) in zip(batch, res):
                        r[2] = (ix[:r[1]], sc[:r[1]], md[:r[1]])
                except BaseException as e:  # every caller of the batch sees the failure
                    for r in batch:
                        r[3] = e
                finally:
                    self._cv.acquire()
                    self._running -= 1
                    self.batches += 1
                    self.queries += len(batch)
                    self._recent.append(len(batch))
                    self._cv.notify_all()
        finally:
            self._cv.release()
        if req[3] is not None:
            raise req[3]
        return req[2]


class MLXVectorStore:
    """service/optimized_vector_store.py:59-242, MI355X-native."""

    def __init__(self, store_path: str, config: Optional[MLXVectorStoreConfig] = None):
        self.store_path = Path(store_path).expanduser()
        self.config = config or MLXVectorStoreConfig()
        self._lock = threading.RLock()  # serialises writers (the reference's lock, :97, :199)
        self._rw = _RWLock()            # queries (shared) vs adds / clear (exclusive)
        self.store_path.mkdir(parents=True, exist_ok=True)
        self._is_dirty = False
        self._compiled_similarity_fn = None
        self._index = None  # _vdb.NativeIndex, or _vdb.NativeShards over config.devices
        self._dim: Optional[int] = None
        self._metadata: List[Dict] = []
        self._meta_index = MetadataIndex()
        self._vector_count = 0
        # query_groups: the one group column attached to the index, (key, rows, update count), its
        # values and the index's "group_sets" when it was attached
        self._group_lock = threading.Lock()
        self._group_tag: Optional[Tuple] = None
        self._group_values: List[Any] = []
        self._group_sets = -1
        # sparse_query / hybrid_query: the one sparse column attached to the index, (key, rows,
        # update count), its n_terms and the index's "sparse_sets" when it was attached
        self._sparse_lock = threading.Lock()
        self._sparse_tag: Optional[Tuple] = None
        self._sparse_terms = 0
        self._sparse_sets = -1
        # range filters: metadata key -> (slot, (rows, update count, metadata version), exact) for the numeric columns
        # attached to the index's 16 slots, least recently used first, and the index's
        # "column_sets" after the last attach made here
        self._column_lock = threading.Lock()
        self._col_slots: "OrderedDict[Any, Tuple[Optional[int], Tuple, bool]]" = OrderedDict()
        self._column_sets = -1
        self._hnsw_index = None
        self._files = StoreFiles(self.store_path)
        self._coalescer = _QueryCoalescer(lambda Q, k, filters=None: self._search_filtered(
                                              Q, k, filters if filters is not None else [None] * Q.shape[0]),
                                          max_inflight=self.config.coalesce_inflight,
                                          linger_us=self.config.coalesce_linger_us)
        if self.config.enable_hnsw:  # service/optimized_vector_store.py:72-78
            from performance.hnsw_index import ProductionHNSWIndex
            self._hnsw_index = ProductionHNSWIndex(self.config.dimension, self.store_path, self.config.metric,
                                                   device=self._devices()[0])
        self._initialize_store()
        if self.config.jit_compile:
            self._compile_critical_functions()
        logger.info("vdb store initialised: %s | HNSW: %s", self.store_path, self.config.enable_hnsw)

    # ---- state -----------------------------------------------------------------
    def _devices(self) -> List[int]:
        return list(self.config.devices) if self.config.devices else [self.config.device]

    def _create_empty_store(self):
        if self._index is not None:
            self._index.clear()
        self._metadata = []
        self._meta_index.clear()
        self._vector_count = 0
        self._is_dirty = False

    def _initialize_store(self):
        self._load_store()

    def _compile_critical_functions(self):
        # the operator slot: which device kernel family serves brute force (:211-213)
        if self.config.metric in _vdb.METRIC_IDS:
            self._compiled_similarity_fn = self.config.metric

    def _ensure_index(self, dim: int):
        if self._index is None:
            metric = self.config.metric if self.config.metric in _vdb.METRIC_IDS else "cosine"
            devs = self._devices()
            if len(devs) > 1:
                # row shards over several GPUs of this process (service/_vdb.py NativeShards)
                self._index = _vdb.NativeShards(dim, metric, devs)
            else:
                self._index = _vdb.NativeIndex(dim, metric, devs[0])
            self._dim = dim
        elif dim != self._dim:
            raise ValueError(f"Dimension mismatch: store holds {self._dim}-d vectors, got {dim}-d")
        return self._index

    @property
    def _vectors(self) -> Optional[np.ndarray]:
        """The corpus as [N, D] float32 (copied back from the GPU), or None if empty."""
        if self._index is None or self._vector_count == 0:
            return None
        return self._index.get_vectors()

    # ---- ingest ------------------------------------------------------------------
    def add_vectors(self, vectors: Union[np.ndarray, Any], metadata: List[Dict]):
        """service/optimized_vector_store.py:96-114."""
        with self._lock, _Write(self._rw):
            return self._add_locked(vectors, metadata)

    def _add_locked(self, vectors, metadata: List[Dict]):
        """add_vectors with the write locks held."""
        v = _as_matrix(vectors)
        if v.ndim == 1:
            v = v[None, :]
        if v.ndim != 2:
            raise ValueError(f"vectors must be 2-D (n, dim), got shape {v.shape}")
        n0 = self._vector_count
        if v.shape[0] > 0:
            self._ensure_index(v.shape[1]).add(v)
        self._metadata.extend(metadata)
        # the filter postings index exactly the rows' metadata (row r <-> metadata[r])
        self._meta_index.extend(self._metadata[len(self._meta_index):])
        self._vector_count = self._index.count() if self._index is not None else 0
        self._is_dirty = True
        if self.config.persist and v.shape[0] > 0:
            # O(new rows) append instead of the reference's full rewrite per add (:113, :218-223)
            self._files.append(v, metadata)
            if self._files.needs_compaction():
                self._save_store(force=True)
            else:
                self._is_dirty = False
        if self.config.enable_hnsw and self._hnsw_index is not None and self._index is not None:
            # the reference rebuilds the graph from scratch on every add (:110-112); the graph
            # path inserts the new rows into the existing graph instead (performance/hnsw_index.py)
            self._hnsw_index.add_rows(self._index, n0)
        return {"vectors_added": len(metadata), "total_vectors": self._vector_count}

    # ---- delete ----------------------------------------------------------------------
    def delete_vectors(self, filter_metadata: Optional[Dict]) -> Dict[str, int]:
        """Delete every row whose metadata matches ``filter_metadata`` (the filter semantics of
        ``query``).  The reference store cannot delete; its Python SDK expects the capability
        (sdk/python/mlx_vector_db_client.py:292-303, POST /vectors/delete).  The rows are
        compacted on the device (include/vdb.h vdb_index_remove); the survivors keep their order
        and are renumbered.  An empty filter raises: ``clear()`` deletes everything."""
        self._check_can_delete()
        if not filter_metadata:
            raise ValueError("delete_vectors needs a non-empty filter_metadata; use clear() to delete everything")
        with self._lock, _Write(self._rw):
            n = self._vector_count
            if n == 0:
                return {"deleted": 0, "total_vectors": 0}
            mask, hits = self._filter_masks([filter_metadata], n)[0]
            if hits == 0:
                return {"deleted": 0, "total_vectors": n}
            return self._delete_locked(mask)

    def delete_rows(self, indices) -> Dict[str, int]:
        """``delete_vectors`` by position: row ids in [0, count), any order."""
        self._check_can_delete()
        with self._lock, _Write(self._rw):
            n = self._vector_count
            ids = np.asarray(indices).reshape(-1)
            if ids.size == 0:
                return {"deleted": 0, "total_vectors": n}
            if ids.dtype.kind not in "iu":
                raise ValueError(f"row ids must be integers, got dtype {ids.dtype}")
            return self._delete_locked(_vdb.rows_to_bitmap(ids.astype(np.int64), n))

    def _check_can_delete(self):
        if len(self._devices()) > 1:
            raise NotImplementedError("delete is not supported on a multi-device store")

    def _delete_locked(self, mask: np.ndarray) -> Dict[str, int]:
        """Remove the rows of a uint32 bitmap over [0, count) (write locks held)."""
        n = self._vector_count
        rows = np.nonzero(np.unpackbits(np.ascontiguousarray(mask, np.uint32).view(np.uint8),
                                        bitorder="little")[:n])[0]
        deleted = self._index.remove(mask)
        gone = set(rows.tolist())
        self._metadata = [m for i, m in enumerate(self._metadata) if i not in gone]
        self._meta_index.remove(rows[rows < len(self._meta_index)])
        self._vector_count = self._index.count()
        if self.config.persist:
            # the reference's cost model, a full rewrite per mutation (:113, :218-223): the base
            # files hold the survivors at once and the append log is dropped
            if self._vector_count:
                self._is_dirty = True
                self._save_store(force=True)
            else:
                self._files.remove_all()
                self._is_dirty = False
        else:
            self._is_dirty = True
        if self.config.enable_hnsw and self._hnsw_index is not None:
            # a graph over the old numbering is stale for good: rebuilt from the index, as the
            # reference rebuilds on every add (:110-112)
            # (an emptied store answers no query; the next add rebuilds: add_rows sees the old count)
            if self._vector_count:
                self._hnsw_index.build(None, native_index=self._index)
        return {"deleted": int(deleted), "total_vectors": self._vector_count}

    # ---- update ----------------------------------------------------------------------
    def update_rows(self, indices, vectors, metadata: Optional[List[Dict]] = None) -> Dict[str, int]:
        """Replace rows in place, by position: row indices[i] becomes vectors[i] (and, with
        ``metadata``, a list of the same length, takes metadata[i]; otherwise the rows keep
        theirs).  No row moves or is renumbered (include/vdb.h vdb_index_update).  Ids outside
        [0, count) or repeated raise ValueError with store and index unchanged."""
        self._check_can_update()
        with self._lock, _Write(self._rw):
            ids, v = self._check_update_args(indices, vectors, metadata)
            if ids.size:
                self._update_locked(ids, v, metadata)
            return {"updated": int(ids.size), "total_vectors": self._vector_count}

    def upsert_vectors(self, vectors, metadata: List[Dict], key: str = "id") -> Dict[str, int]:
        """Insert or replace by ``metadata[key]``: an item whose key value one stored row holds
        replaces that row's vector and metadata in place (one device update for all such items);
        the others are appended in their given order (one add).  The reference store has no
        counterpart; its benchmark calls ``upsert`` on the database it compares itself with
        (benchmarks/benchmark_app.py:104).  Raises ValueError before anything changes for an item
        without ``key``, two items with the same key value, or a key value more than one stored
        row holds."""
        self._check_can_update()
        with self._lock, _Write(self._rw):
            v = _as_matrix(vectors)
            if v.ndim == 1:
                v = v[None, :]
            if v.ndim != 2:
                raise ValueError(f"vectors must be 2-D (n, dim), got shape {v.shape}")
            if len(metadata) != v.shape[0]:
                raise ValueError(f"{v.shape[0]} vectors but {len(metadata)} metadata entries")
            if self._dim is not None and v.shape[0] and v.shape[1] != self._dim:
                raise ValueError(f"Dimension mismatch: store holds {self._dim}-d vectors, got {v.shape[1]}-d")
            seen = set()
            hit_items, hit_rows, new_items = [], [], []
            for i, m in enumerate(metadata):
                if not isinstance(m, dict) or key not in m:
                    raise ValueError(f"upsert item {i} has no metadata key {key!r}")
                kv = m[key]
                try:
                    dup = kv in seen
                    seen.add(kv)
                except TypeError:
                    raise ValueError(f"upsert item {i}: {key!r} value {kv!r} is not hashable") from None
                if dup:
                    raise ValueError(f"upsert items share the {key!r} value {kv!r}")
                rows = self._meta_index.rows_with(key, kv)
                if rows.size > 1:
                    raise ValueError(f"{rows.size} stored rows hold the {key!r} value {kv!r}")
                if rows.size == 1:
                    hit_items.append(i)
                    hit_rows.append(int(rows[0]))
                else:
                    new_items.append(i)
            if not np.isfinite(v).all():  # (the device would reject the update or the add alone)
                raise ValueError("vectors contain NaN or Inf; nothing was changed")
            if hit_items:
                self._update_locked(np.asarray(hit_rows, np.int64), v[hit_items], [metadata[i] for i in hit_items],
                                    save=not new_items)
            if new_items:
                self._add_locked(v[new_items], [metadata[i] for i in new_items])
                if hit_items and self.config.persist:
                    # the append log cannot record an update: the base files take both at once
                    self._is_dirty = True
                    self._save_store(force=True)
            return {"updated": len(hit_items), "added": len(new_items), "total_vectors": self._vector_count}

    def _check_can_update(self):
        if len(self._devices()) > 1:
            raise NotImplementedError("update is not supported on a multi-device store")

    def _check_update_args(self, indices, vectors, metadata) -> Tuple[np.ndarray, np.ndarray]:
        n = self._vector_count
        ids = np.asarray(indices).reshape(-1)
        if ids.size and ids.dtype.kind not in "iu":
            raise ValueError(f"row ids must be integers, got dtype {ids.dtype}")
        ids = ids.astype(np.int64)
        v = _as_matrix(vectors)
        if v.ndim == 1:
            v = v[None, :]
        if v.ndim != 2 or v.shape[0] != ids.size:
            raise ValueError(f"vectors must have shape ({ids.size}, dim), got {v.shape}")
        if metadata is not None and len(metadata) != ids.size:
            raise ValueError(f"{ids.size} rows but {len(metadata)} metadata entries")
        if ids.size:
            if int(ids.min()) < 0 or int(ids.max()) >= n:
                raise ValueError(f"row ids must be in [0, {n}), got [{int(ids.min())}, {int(ids.max())}]")
            if np.unique(ids).size != ids.size:
                raise ValueError("row ids must be pairwise distinct")
            if v.shape[1] != self._dim:
                raise ValueError(f"Dimension mismatch: store holds {self._dim}-d vectors, got {v.shape[1]}-d")
        return ids, v

    def _update_locked(self, ids: np.ndarray, v: np.ndarray, metadata: Optional[List[Dict]], save: bool = True):
        """Rows ids := v on the device, then their metadata (write locks held, arguments checked:
        the device call rejects what is left, a non-finite value, before it writes)."""
        self._index.update(ids, v)
        if metadata is not None:
            if len(self._metadata) < self._vector_count:
                self._metadata.extend({} for _ in range(self._vector_count - len(self._metadata)))
            for r, m in zip(ids.tolist(), metadata):
                self._metadata[r] = m
            self._meta_index.replace(ids, metadata)
        self._is_dirty = True
        if self.config.persist and save:
            # delete's cost model: a full rewrite of the base files (the append log has no update record)
            self._save_store(force=True)
        if self.config.enable_hnsw and self._hnsw_index is not None and self._vector_count:
            # the graph is stale by generation: rebuilt from the index, as after a delete
            self._hnsw_index.build(None, native_index=self._index)

    # ---- query ---------------------------------------------------------------------
    def query(self, query_vector: Union[np.ndarray, Any], k: int = 10,
              filter_metadata: Optional[Dict] = None, use_hnsw: bool = True) -> Tuple:
        """service/optimized_vector_store.py:116-145 -> (indices, scores, metadata)."""
        with _Read(self._rw):
            if self._vector_count == 0:
                return [], [], []
            q = _as_matrix(query_vector)
            if q.ndim == 2 and q.shape[0] == 1:
                q = q[0]
            if q.ndim != 1:
                raise ValueError(f"query takes one vector of shape (dim,) or (1, dim), got {q.shape}; "
                                 "use batch_query for several")
            h = self._hnsw_index
            if use_hnsw and self.config.enable_hnsw and h is not None and h.is_loaded:
                # service/optimized_vector_store.py:120-143: hnswlib distances, k*10 candidates
                # when filtering, brute force on any failure
                # (the filter is parsed once, outside the try: a malformed condition is the caller's error)
                matches = filter_ops.compile_filter(filter_metadata) if filter_metadata else None
                try:
                    candidate_k = k * 10 if filter_metadata else k
                    indices, distances = h.search(q[None, :], k=candidate_k)
                    indices, distances = indices[0], distances[0]
                    if not filter_metadata:
                        return ([int(i) for i in indices], distances.tolist(),
                                [self._metadata[int(i)] for i in indices])
                    hits = []
                    for i, idx in enumerate(indices):
                        if idx < len(self._metadata):
                            meta = self._metadata[int(idx)]
                            if matches(meta):
                                hits.append((int(idx), float(distances[i]), meta))
                        if len(hits) == k:
                            break
                    if not hits:
                        return [], [], []
                    fi, fd, fm = zip(*hits)
                    return list(fi), list(fd), list(fm)
                except Exception as e:
                    logger.warning("HNSW-Suche fehlgeschlagen, falle auf Brute-Force zurück: %s", e)
            # k above the device limit is not coalesced: its error is the caller's alone
            if self.config.coalesce and self._compiled_similarity_fn and 0 < int(k) <= 1024:
                if q.shape[0] != self._dim:
                    raise ValueError(f"Dimension mismatch: query has {q.shape[0]} dims, store holds {self._dim}")
                if not filter_metadata:
                    return self._coalescer.query(q, k)
                # a filter the planner searches as a row list joins a batch of such filters (one
                # device call for all of them); any other keeps its own masked search
                # (a filter with range operators is evaluated once, by the planner below: its mask
                # is cached nowhere, so a look at its count here would be a second device call)
                if not filter_ops.has_range_ops(filter_metadata):
                    eligible = self._filter_masks([filter_metadata], self._vector_count)[0][1]
                    if eligible == 0:
                        return [], [], []
                    if self._subset_ok(eligible):
                        return self._coalescer.query(q, k, filter_metadata)
            return self._brute_force_search(q[None, :], k, filter_metadata)[0]

    def batch_query(self, query_vectors: Union[np.ndarray, Any], k: int = 10,
                    filter_metadata: Optional[Union[Dict, List[Optional[Dict]]]] = None) -> List[Tuple]:
        """The batched path (performance/mlx_optimized.py:217-248) behind the store API that
        api/routes/vectors.py:291 and tests/demo.py:134-137 call: one (indices, distances,
        metadata) tuple per query, same rows and order as ``query`` for that vector.

        The second element is a DISTANCE, because that is how its only caller reads it:
        /vectors/batch_query unpacks ``indices, distances, metadata_list`` and scores cosine
        as ``max(0, 1.0 - dist)`` and euclidean as ``1 / (1 + dist)``
        (api/routes/vectors.py:300-306).  So cosine returns ``1 - cos`` and euclidean the
        sqrt-L2 distance (which is what ``query`` already returns for euclidean).

        ``filter_metadata``: one dict for every query, or a list of B dicts / Nones, one filter
        per query (the reference's multi-tenant use: each request its own user / model filter)."""
        q = _as_matrix(query_vectors)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2:
            raise ValueError(f"query_vectors must be 2-D (B, dim), got {q.shape}")
        per_query = isinstance(filter_metadata, (list, tuple))
        if per_query and len(filter_metadata) != q.shape[0]:
            raise ValueError(f"{q.shape[0]} queries but {len(filter_metadata)} filters")
        with _Read(self._rw):
            if self._vector_count == 0 or q.shape[0] == 0:
                return [([], [], []) for _ in range(q.shape[0])]
            if per_query:
                res = self._search_filtered(q, k, list(filter_metadata))
            else:
                res = self._brute_force_search(q, k, filter_metadata)
        if self.config.metric == "cosine":
            res = [(i, [1.0 - s for s in sc], m) for i, sc, m in res]
        return res

    def _brute_force_search(self, Q: np.ndarray, k: int, filter_metadata: Optional[Dict] = None):
        """service/optimized_vector_store.py:149-192 for a [B, D] block of queries
        (called with the read lock held): the planner with one filter for every query."""
        return self._search_filtered(Q, k, [filter_metadata] * Q.shape[0])

    def _subset_ok(self, eligible: int) -> bool:
        """A filter with ``eligible`` matching rows is searched as a row list (the planner's rule)."""
        frac = float(self.config.subset_max_fraction)
        return (frac > 0.0 and len(self._devices()) == 1 and hasattr(self._index, "search_rows")
                and eligible <= frac * self._vector_count)

    # ---- filter operators ------------------------------------------------------------
    def _filter_masks(self, filters: List[Dict], n: int) -> List[Tuple[np.ndarray, int]]:
        """(uint32 words over rows [0, n), eligible count) for each filter (read or write lock
        held): the one place a filter becomes a row_mask.  A filter without conditions
        (service/filter_ops.py) is exactly ``MetadataIndex.bitmap``, cache included.  A filter
        with range operators is split: its pairs and posting operators ($eq, $ne, $in, $nin,
        $exists) are a host bitmap, the predicate's base mask, and the range operators of each key
        fold into one clause on that key's numeric column; all such filters of the call go into
        ONE ``filter_mask`` call (include/vdb.h vdb_index_filter_mask), a predicate each, in
        chunks of 256.  The host evaluates the range operators instead on a multi-device store,
        when a column or a bound is not exact in fp64 or a filter needs more than 8 clauses: the
        answer is the same either way."""
        out: List[Optional[Tuple[np.ndarray, int]]] = [None] * len(filters)
        dev = []  # (position, the filter, its base filter, {key: folded interval})
        for i, f in enumerate(filters):
            plain, conds = filter_ops.split_filter(f)  # (a malformed condition raises here)
            ranges = {k: filter_ops.fold_range(filter_ops.range_ops(ops)) for k, ops in conds.items()
                      if filter_ops.range_ops(ops)}
            if not ranges or not self._device_filter_ok(ranges, n):
                out[i] = self._meta_index.bitmap(f, n)
                continue
            base = dict(plain)
            for k, ops in conds.items():
                post = filter_ops.posting_ops(ops)
                if post:
                    base[k] = dict(post)
            dev.append((i, f, base, ranges))
        chunk, keys = [], set()
        for item in dev:
            more = keys | set(item[3])
            if chunk and (len(chunk) == _vdb.FILTER_MAX_PREDS or len(more) > _vdb.FILTER_SLOTS):
                self._device_filter_chunk(chunk, n, out)
                chunk, more = [], set(item[3])
            chunk.append(item)
            keys = more
        if chunk:
            self._device_filter_chunk(chunk, n, out)
        return out

    def _filter_rows(self, filt: Dict, mask: np.ndarray, n: int) -> np.ndarray:
        """The ascending row list of a filter whose mask ``_filter_masks`` gave: from the postings
        in O(matching rows) as ever for a filter without range operators, off the mask's non-zero
        words for one with them (its rows exist nowhere else; evaluating it again would cost more)."""
        if filter_ops.has_range_ops(filt):
            return _mask_rows(mask, n)
        return self._meta_index.rows(filt, n)

    def _device_filter_ok(self, ranges: Dict, n: int) -> bool:
        """The device takes these range clauses: a single-device store with rows, at most 8 keys
        and every bound unchanged by the conversion to fp64 (the columns are checked at attach)."""
        return (n > 0 and len(self._devices()) == 1 and hasattr(self._index, "filter_mask")
                and len(ranges) <= _vdb.FILTER_MAX_CLAUSES
                and all(filter_ops.float_exact(lo) and filter_ops.float_exact(hi) for lo, _, hi, _ in ranges.values()))

    def _attach_columns(self, keys, n: int) -> Dict[Any, Optional[int]]:
        """Make every key's numeric column one of the index's 16 (``_column_lock`` held) -> key ->
        slot, None for a key whose column is not exact in fp64.  An entry is kept while the row
        count and the rows' contents stay as they were and the index still holds what was attached
        here (an add, a delete and a clear drop the slots; an upsert may change a value; the
        metadata index's version moves with each of them, so a key found inexact is looked at again
        once the rows have changed).  The table holds at most 16 keys, inexact ones included: the
        least recently used gives way to a 17th."""
        tag = (n, self._index.stat("rows_updated"), self._meta_index.version)
        sets = self._index.stat("column_sets")
        if sets != self._column_sets:
            self._col_slots.clear()  # somebody else attached a column: nothing here is known to hold
            self._column_sets = sets
        held = self._index.stat("column_slots")
        for key in [k for k, (slot, t, _) in self._col_slots.items()
                    if t != tag or (slot is not None and not (held >> slot) & 1)]:
            del self._col_slots[key]
        slots: Dict[Any, Optional[int]] = {}
        for key in keys:
            if key in self._col_slots:
                self._col_slots.move_to_end(key)
                slots[key] = self._col_slots[key][0]
                continue
            col, exact = self._meta_index.numeric_column(key, n)
            slot = None
            while len(self._col_slots) >= _vdb.FILTER_SLOTS:
                victim = next(k for k in self._col_slots if k not in keys)
                del self._col_slots[victim]
            if exact:
                used = {s for s, _, _ in self._col_slots.values()}
                slot = next(s for s in range(_vdb.FILTER_SLOTS) if s not in used)
                self._index.set_column(slot, col)
                self._column_sets = self._index.stat("column_sets")
            self._col_slots[key] = (slot, tag, exact)
            slots[key] = slot
        return slots

    def _device_filter_chunk(self, chunk, n: int, out: List) -> None:
        """One ``filter_mask`` call for up to 256 filters with range clauses (at most 16 keys
        between them); a filter on a column that is not exact goes to the host instead."""
        W = (n + 31) // 32
        keys = sorted({k for _, _, _, ranges in chunk for k in ranges}, key=repr)
        with self._column_lock:  # attach and evaluate as one step: no other reader evicts a slot in between
            slots = self._attach_columns(keys, n)
            preds, bases, where = [], [], []
            for i, f, base, ranges in chunk:
                if any(slots[k] is None for k in ranges):
                    out[i] = self._meta_index.bitmap(f, n)
                    continue
                if base:
                    words, eligible = self._meta_index.bitmap(base, n)
                    if eligible == 0:
                        out[i] = (np.zeros(W, np.uint32), 0)
                        continue
                else:
                    words = None
                preds.append([(slots[k], float(lo), float(hi),
                               (_vdb.FILTER_LO_INCL if li else 0) | (_vdb.FILTER_HI_INCL if hi_i else 0))
                              for k, (lo, li, hi, hi_i) in ranges.items()])
                bases.append(words)
                where.append(i)
            if not preds:
                return
            base_masks = None
            if any(b is not None for b in bases):
                base_masks = np.empty((len(preds), W), np.uint32)
                for p, b in enumerate(bases):
                    base_masks[p] = 0xFFFFFFFF if b is None else b[:W]
            masks, counts = self._index.filter_mask(preds, base_masks)
        for p, i in enumerate(where):
            out[i] = (masks[p], int(counts[p]))

    def count_matching(self, filter_metadata: Optional[Dict]) -> int:
        """How many stored rows match ``filter_metadata`` (the filter semantics of ``query``,
        conditions included); without a filter, the number of rows."""
        with _Read(self._rw):
            n = self._vector_count
            if n == 0 or not filter_metadata:
                if filter_metadata:
                    filter_ops.split_filter(filter_metadata)  # (still checked)
                return n
            return int(self._filter_masks([filter_metadata], n)[0][1])

    def _search_filtered(self, Q: np.ndarray, k: int, filters: List[Optional[Dict]]):
        """The planner of every brute-force read (called with the read lock held): ``filters``
        holds one entry per query, a dict or None.  Queries are grouped by filter.  A group without
        a filter, one whose eligible rows exceed ``subset_max_fraction`` of the store and any group
        on a multi-device store take one ``search`` each (row_mask = the filter's bitmap); all
        other groups go into ONE ``search_rows`` call, one row list per distinct filter.  Both
        device paths rank by the same exact keys, so the choice never shows in the results."""
        if not self._compiled_similarity_fn:
            raise RuntimeError(_NO_OPERATOR_MSG)
        B = Q.shape[0]
        if Q.shape[1] != self._dim:
            raise ValueError(f"Dimension mismatch: query has {Q.shape[1]} dims, store holds {self._dim}")
        if len(filters) != B:
            raise ValueError(f"{B} queries but {len(filters)} filters")
        k = int(k)
        if k <= 0:
            return [([], [], []) for _ in range(B)]
        n = self._vector_count
        out: List[Optional[Tuple]] = [None] * B
        groups: Dict[Any, Tuple[Optional[Dict], List[int]]] = {}
        for b, f in enumerate(filters):
            groups.setdefault(_filter_key(f) if f else None, (f if f else None, []))[1].append(b)
        masked, subset = [], []
        # posting lists maintained at add time, not the reference's O(N) scan (:159-165); the range
        # clauses of all the groups that carry any in one device call (_filter_masks)
        filtered = [(filt, members) for filt, members in groups.values() if filt is not None]
        bitmaps = self._filter_masks([filt for filt, _ in filtered], n)
        for filt, members in groups.values():
            if filt is None:
                masked.append((None, n, members))
        for (filt, members), (mask, eligible) in zip(filtered, bitmaps):
            if eligible == 0:
                for b in members:
                    out[b] = ([], [], [])
            elif self._subset_ok(eligible):
                subset.append((filt, mask, eligible, members))
            else:
                masked.append((mask, eligible, members))

        def fill(members, scores, idx):
            meta = self._metadata
            for j, b in enumerate(members):
                valid = idx[j] >= 0
                ib = idx[j][valid].tolist()
                sb = scores[j][valid].astype(np.float64).tolist()
                out[b] = (ib, sb, [meta[i] if i < len(meta) else {} for i in ib])

        def take(members):
            return Q if members == list(range(B)) else Q[members]  # (one group: Q as it is)

        for mask, eligible, members in masked:
            kk = min(k, eligible)
            if kk > 1024:
                raise ValueError(f"k={k} exceeds the device top-k limit of 1024")
            scores, idx = self._index.search(take(members), kk, row_mask=mask)
            fill(members, scores, idx)
        if subset:
            kk = min(k, max(e for _, _, e, _ in subset))  # (a shorter list pads its rows with -1)
            if kk > 1024:
                raise ValueError(f"k={k} exceeds the device top-k limit of 1024")
            members = [b for _, _, _, mem in subset for b in mem]
            lists = [self._filter_rows(filt, mask, n) for filt, mask, _, _ in subset]
            qlist = np.concatenate([np.full(len(mem), li, np.int32) for li, (_, _, _, mem) in enumerate(subset)])
            scores, idx = self._index.search_rows(take(members), kk, lists, query_list=qlist)
            fill(members, scores, idx)
        return out

    # ---- range query ----------------------------------------------------------------
    def range_query(self, query_vector: Union[np.ndarray, Any], threshold: float,
                    filter_metadata: Optional[Dict] = None, limit: Optional[int] = None,
                    with_total: bool = False) -> Tuple:
        """Every stored row within ``threshold`` of the query -> (indices, scores, metadata), best
        first: cosine rows with similarity >= threshold, score descending; euclidean rows with
        distance <= threshold, distance ascending; ties to the lower row, the order ``query``
        uses, and the scores ``query`` returns.  ``limit`` keeps the best ``limit`` after sorting.
        Exact (include/vdb.h vdb_index_search_range), and not capped at 1024 results as ``query``
        is.  The reference has no such read: its RAG pipeline fetches k * 2 and drops what is under
        min_similarity (integrations/mlx_lm_pipeline.py:725-736).  ``with_total``: a fourth element,
        the exact number of rows within the threshold (what ``count_within`` returns), from the
        same device call: with a ``limit`` only the best ``limit`` entries are built."""
        q = _as_matrix(query_vector)
        if q.ndim == 2 and q.shape[0] == 1:
            q = q[0]
        if q.ndim != 1:
            raise ValueError(f"range_query takes one vector of shape (dim,) or (1, dim), got {q.shape}; "
                             "use batch_range_query for several")
        res = self._range_search(q[None, :], [threshold], filter_metadata, limit)[0]
        return res if with_total else res[:3]

    def batch_range_query(self, query_vectors: Union[np.ndarray, Any], thresholds,
                          filter_metadata: Optional[Dict] = None) -> List[Tuple]:
        """``range_query`` for a [B, dim] block of queries from one device call: one (indices,
        scores, metadata) tuple per query.  ``thresholds``: one per query, or a scalar for all."""
        q = _as_matrix(query_vectors)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2:
            raise ValueError(f"query_vectors must be 2-D (B, dim), got {q.shape}")
        thr = np.asarray(thresholds, dtype=np.float64)
        thr = np.full(q.shape[0], float(thr)) if thr.ndim == 0 else thr.reshape(-1)
        if thr.size != q.shape[0]:
            raise ValueError(f"{q.shape[0]} queries but {thr.size} thresholds")
        return [r[:3] for r in self._range_search(q, thr, filter_metadata, None)]

    def count_within(self, query_vector: Union[np.ndarray, Any], threshold: float,
                     filter_metadata: Optional[Dict] = None) -> int:
        """How many stored rows ``range_query`` would return, from a count-only device call."""
        q = _as_matrix(query_vector)
        if q.ndim == 2 and q.shape[0] == 1:
            q = q[0]
        if q.ndim != 1:
            raise ValueError(f"count_within takes one vector of shape (dim,) or (1, dim), got {q.shape}")
        self._check_can_range()
        with _Read(self._rw):
            mask = self._range_mask(q[None, :], filter_metadata)
            if mask is False:
                return 0
            return int(self._index.search_range(q[None, :], [float(threshold)], cap=0, row_mask=mask)[0][0])

    def _check_can_range(self):
        if len(self._devices()) > 1:
            raise NotImplementedError("range query is not supported on a multi-device store")

    def _range_mask(self, Q: np.ndarray, filter_metadata: Optional[Dict]):
        """The row_mask of a range read (read lock held): None without a filter, False when the
        store is empty or nothing matches the filter (no device call is needed)."""
        if self._vector_count == 0:
            return False
        if not self._compiled_similarity_fn:
            raise RuntimeError(_NO_OPERATOR_MSG)
        if Q.shape[1] != self._dim:
            raise ValueError(f"Dimension mismatch: query has {Q.shape[1]} dims, store holds {self._dim}")
        if not filter_metadata:
            return None
        mask, eligible = self._filter_masks([filter_metadata], self._vector_count)[0]
        return mask if eligible else False

    def _range_search(self, Q: np.ndarray, thresholds, filter_metadata: Optional[Dict], limit: Optional[int]):
        """One (indices, scores, metadata, total) tuple per query; total = the exact hit count."""
        self._check_can_range()
        if limit is not None and int(limit) < 0:
            raise ValueError(f"limit must be >= 0, got {limit}")
        with _Read(self._rw):
            mask = self._range_mask(Q, filter_metadata)
            if mask is False:
                return [([], [], [], 0) for _ in range(Q.shape[0])]
            thr = np.asarray(thresholds, dtype=np.float64)
            counts, idx, scores, keys = self._index.search_range(Q, thr, row_mask=mask, with_keys=True)
            meta = self._metadata
            out = []
            for b in range(Q.shape[0]):
                n = int(counts[b])
                order = np.lexsort((idx[b, :n], -keys[b, :n]))  # key descending, ties to the lower row
                if limit is not None:
                    order = order[:int(limit)]
                ib = idx[b, :n][order].tolist()
                sb = scores[b, :n][order].astype(np.float64).tolist()
                out.append((ib, sb, [meta[i] if i < len(meta) else {} for i in ib], n))
            return out

    # ---- grouped query ---------------------------------------------------------------
    def query_groups(self, query_vector: Union[np.ndarray, Any], group_by: str, k: int = 10, group_size: int = 1,
                     filter_metadata: Optional[Dict] = None) -> List[Dict]:
        """The ``k`` best distinct values of the metadata key ``group_by`` ("the k best documents,
        with the best chunk of each") -> a list of ``{"group": value, "hits": (indices, scores,
        metadata)}``, best group first; the hits are in the form ``query`` returns them, best
        first, at most ``group_size`` per group.  A group ranks by its best row (the exact key
        ``query`` ranks by, ties to the lower row); rows without the key belong to no group.
        Exact (include/vdb.h vdb_index_search_groups): no over-fetch that one long document can
        fill.  The reference has no such read: its RAG pipeline stores document_id beside every
        chunk (integrations/mlx_lm_pipeline.py:656-670) and asks for the best k chunks."""
        q = _as_matrix(query_vector)
        if q.ndim == 2 and q.shape[0] == 1:
            q = q[0]
        if q.ndim != 1:
            raise ValueError(f"query_groups takes one vector of shape (dim,) or (1, dim), got {q.shape}; "
                             "use batch_query_groups for several")
        return self._group_search(q[None, :], group_by, k, group_size, filter_metadata)[0]

    def batch_query_groups(self, query_vectors: Union[np.ndarray, Any], group_by: str, k: int = 10,
                           group_size: int = 1, filter_metadata: Optional[Dict] = None) -> List[List[Dict]]:
        """``query_groups`` for a [B, dim] block of queries: one list of groups per query, from one
        device call (two with ``group_size`` > 1)."""
        q = _as_matrix(query_vectors)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2:
            raise ValueError(f"query_vectors must be 2-D (B, dim), got {q.shape}")
        return self._group_search(q, group_by, k, group_size, filter_metadata)

    def _attach_groups(self, group_by) -> List[Any]:
        """Make ``group_by``'s column the one attached to the index (read lock and _group_lock
        held) -> its values, group id = position.  Kept while the key, the row count and the
        rows' contents stay as they were and the index still holds it (an add, a delete and a
        clear drop it; an upsert may change a row's value)."""
        n = self._vector_count
        tag = (group_by, n, self._index.stat("rows_updated"))
        if self._group_tag == tag and self._index.stat("group_rows") == n \
                and self._index.stat("group_sets") == self._group_sets:
            return self._group_values
        col, values = self._meta_index.group_column(group_by, n)
        self._group_tag = None
        if not values:  # no row has the key: nothing is searched, and no other key's column stays attached
            if self._index.stat("group_rows"):
                self._index.set_groups(None)
        else:
            self._index.set_groups(col)
            self._group_tag, self._group_values = tag, values
            self._group_sets = self._index.stat("group_sets")
        return values

    def _group_search(self, Q: np.ndarray, group_by, k: int, group_size: int, filter_metadata: Optional[Dict]):
        if len(self._devices()) > 1:
            raise NotImplementedError("grouped query is not supported on a multi-device store")
        k, group_size = int(k), int(group_size)
        if not 1 <= k <= GROUP_MAX_K:
            raise ValueError(f"k must be in [1, {GROUP_MAX_K}], got {k}")
        if not 1 <= group_size <= GROUP_MAX_SIZE:
            raise ValueError(f"group_size must be in [1, {GROUP_MAX_SIZE}], got {group_size}")
        B = Q.shape[0]
        with _Read(self._rw):
            # (never the graph path, never the coalescer: one exact device call for the block)
            mask = self._range_mask(Q, filter_metadata)  # None: no filter; False: nothing to search
            if mask is False or B == 0:
                return [[] for _ in range(B)]
            n = self._vector_count
            with self._group_lock:  # one attached column: attach and search as one step
                values = self._attach_groups(group_by)
                if not values:  # no row has the key
                    return [[] for _ in range(B)]
                scores, idx, grp = self._index.search_groups(Q, k, row_mask=mask)
            meta = self._metadata

            def hits_of(rows, sc):
                return (rows, sc, [meta[i] if i < len(meta) else {} for i in rows])

            out = []
            if group_size == 1:
                for b in range(B):
                    valid = idx[b] >= 0
                    out.append([{"group": values[g], "hits": hits_of([int(i)], [float(s)])}
                                for i, s, g in zip(idx[b][valid], scores[b][valid].astype(np.float64), grp[b][valid])])
                return out
            # group_size > 1: every returned group's own rows, searched as row lists (one list per
            # distinct group of the batch, shared between the queries that returned it)
            filt_rows = self._filter_rows(filter_metadata, mask, n) if filter_metadata else None
            list_of: Dict[int, int] = {}
            lists, members, qlist = [], [], []
            for b in range(B):
                for g in grp[b][idx[b] >= 0].tolist():
                    if g not in list_of:
                        rows = self._meta_index.rows_with(group_by, values[g])
                        rows = rows[rows < n]
                        if filt_rows is not None:
                            rows = np.intersect1d(rows, filt_rows, assume_unique=True)
                        list_of[g] = len(lists)
                        lists.append(rows)
                    members.append(b)
                    qlist.append(list_of[g])
            if not members:
                return [[] for _ in range(B)]
            kk = min(group_size, max(r.size for r in lists))
            s2, i2 = self._index.search_rows(Q[members], kk, lists, query_list=np.asarray(qlist, np.int32))
            out = [[] for _ in range(B)]
            gids = [g for b in range(B) for g in grp[b][idx[b] >= 0].tolist()]
            for j, (b, g) in enumerate(zip(members, gids)):
                valid = i2[j] >= 0
                out[b].append({"group": values[g],
                               "hits": hits_of(i2[j][valid].tolist(), s2[j][valid].astype(np.float64).tolist())})
            return out

    # ---- MMR query ---------------------------------------------------------------------
    def mmr_query(self, query_vector: Union[np.ndarray, Any], k: int = 10, fetch_k: Optional[int] = None,
                  lambda_mult: float = 0.5, filter_metadata: Optional[Dict] = None) -> Tuple:
        """``k`` rows that are relevant to the query and unlike each other (maximal marginal
        relevance) -> (indices, scores, metadata) as ``query`` returns them, in pick order.  Of the
        best ``fetch_k`` rows (``None``: min(200, max(4 k, 20))) each pick maximises ``lambda_mult *
        relevance - (1 - lambda_mult) * (greatest similarity to a row picked before)``; both terms
        are the exact ranking keys (cosine similarity; minus the SQUARED distance for euclidean), so
        ``lambda_mult`` = 1 is ``query`` and 0 looks at diversity alone.  Exact and the same for
        every precision (include/vdb.h vdb_index_search_mmr).  The reference has no such read: its
        RAG context fills with overlapping chunks of one paragraph
        (integrations/mlx_lm_pipeline.py:646-756)."""
        q = _as_matrix(query_vector)
        if q.ndim == 2 and q.shape[0] == 1:
            q = q[0]
        if q.ndim != 1:
            raise ValueError(f"mmr_query takes one vector of shape (dim,) or (1, dim), got {q.shape}; "
                             "use batch_mmr_query for several")
        return self._mmr_search(q[None, :], k, fetch_k, lambda_mult, filter_metadata)[0]

    def batch_mmr_query(self, query_vectors: Union[np.ndarray, Any], k: int = 10, fetch_k: Optional[int] = None,
                        lambda_mult: float = 0.5, filter_metadata: Optional[Dict] = None) -> List[Tuple]:
        """``mmr_query`` for a [B, dim] block of queries from one device call: one (indices, scores,
        metadata) tuple per query."""
        q = _as_matrix(query_vectors)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2:
            raise ValueError(f"query_vectors must be 2-D (B, dim), got {q.shape}")
        return self._mmr_search(q, k, fetch_k, lambda_mult, filter_metadata)

    def _mmr_search(self, Q: np.ndarray, k, fetch_k, lambda_mult, filter_metadata: Optional[Dict]):
        if len(self._devices()) > 1:
            raise NotImplementedError("MMR query is not supported on a multi-device store")
        k = int(k)
        if not 1 <= k <= MMR_MAX_K:
            raise ValueError(f"k must be in [1, {MMR_MAX_K}], got {k}")
        fetch_k = min(MMR_MAX_FETCH, max(4 * k, 20)) if fetch_k is None else int(fetch_k)
        if not k <= fetch_k <= MMR_MAX_FETCH:
            raise ValueError(f"fetch_k must be in [k, {MMR_MAX_FETCH}], got fetch_k={fetch_k} k={k}")
        lam = float(lambda_mult)
        if not 0.0 <= lam <= 1.0:  # (a NaN fails both comparisons)
            raise ValueError(f"lambda_mult must be in [0, 1], got {lambda_mult}")
        B = Q.shape[0]
        with _Read(self._rw):
            # (never the graph path, never the coalescer: one exact device call for the block)
            mask = self._range_mask(Q, filter_metadata)  # None: no filter; False: nothing to search
            if mask is False or B == 0:
                return [([], [], []) for _ in range(B)]
            scores, idx = self._index.search_mmr(Q, k, fetch_k, lam, row_mask=mask)
            meta = self._metadata
            out = []
            for b in range(B):
                valid = idx[b] >= 0
                ib = idx[b][valid].tolist()
                out.append((ib, scores[b][valid].astype(np.float64).tolist(),
                            [meta[i] if i < len(meta) else {} for i in ib]))
            return out

    # ---- fused query -------------------------------------------------------------------
    def fused_query(self, query_vectors: Union[np.ndarray, Any], k: int = 10, fusion: str = "rrf", weights=None,
                    fetch_k: Optional[int] = None, rrf_c: float = 60.0,
                    filter_metadata: Optional[Dict] = None) -> Tuple:
        """One ranked list from several query vectors ([m, dim], m <= 16: paraphrases of a question,
        the question plus a hypothetical answer, a title and a body embedding) -> (indices, scores,
        metadata, fused, hits), best first: as ``mmr_query``'s tuple, then each row's fused value
        (fp64) and the number of the m lists that held it.  Each vector's best ``fetch_k`` rows
        (``None``: min(200, max(k, 4 k))) are fused per row: ``fusion="rrf"`` adds ``weights[l] /
        (rrf_c + rank)`` over the lists holding the row in list order (``weights`` None: all 1.0);
        ``"max"`` takes its greatest exact key ("the best match to any of the vectors", exact over
        the whole corpus; no weights).  Ties go to the lower row id.  Exact and the same for every
        precision (include/vdb.h vdb_index_search_fused).  The reference has no such read."""
        q = _as_matrix(query_vectors)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2:
            raise ValueError(f"fused_query takes one set of vectors of shape (m, dim), got {q.shape}; "
                             "use batch_fused_query for several sets")
        return self.batch_fused_query([q], k, fusion, None if weights is None else [weights], fetch_k, rrf_c,
                                      filter_metadata)[0]

    def batch_fused_query(self, query_sets, k: int = 10, fusion: str = "rrf", weights=None,
                          fetch_k: Optional[int] = None, rrf_c: float = 60.0,
                          filter_metadata: Optional[Dict] = None) -> List[Tuple]:
        """``fused_query`` for a list of query sets from one device call: one (indices, scores,
        metadata, fused, hits) tuple per set.  ``weights``: None, or one sequence per set."""
        if len(self._devices()) > 1:
            raise NotImplementedError("fused query is not supported on a multi-device store")
        k = int(k)
        if not 1 <= k <= FUSED_MAX_K:
            raise ValueError(f"k must be in [1, {FUSED_MAX_K}], got {k}")
        fetch_k = min(FUSED_MAX_FETCH, max(k, 4 * k)) if fetch_k is None else int(fetch_k)
        if not k <= fetch_k <= FUSED_MAX_FETCH:
            raise ValueError(f"fetch_k must be in [k, {FUSED_MAX_FETCH}], got fetch_k={fetch_k} k={k}")
        if fusion not in _vdb.FUSION_IDS:
            raise ValueError(f"fusion must be one of {sorted(_vdb.FUSION_IDS)}, got {fusion!r}")
        c = float(rrf_c)
        if fusion == "rrf" and not 0.0 <= c < float("inf"):  # (a NaN fails both comparisons)
            raise ValueError(f"rrf_c must be finite and >= 0, got {rrf_c}")
        sets = []
        for s in query_sets:
            a = _as_matrix(s)
            if a.size == 0:  # a set without a vector: no error, no result
                a = np.zeros((0, 0), np.float32)
            elif a.ndim == 1:
                a = a[None, :]
            if a.ndim != 2:
                raise ValueError(f"a query set must be 2-D (m, dim), got {a.shape}")
            if a.shape[0] > FUSED_MAX_LISTS:
                raise ValueError(f"a query set takes at most {FUSED_MAX_LISTS} vectors, got {a.shape[0]}")
            sets.append(a)
        B = len(sets)
        w = None
        if weights is not None:
            if fusion == "max":
                raise ValueError("weights are not used with fusion='max'")
            weights = list(weights)
            if len(weights) != B:
                raise ValueError(f"weights needs one sequence per query set ({B}), got {len(weights)}")
            ws = [np.asarray(x, dtype=np.float64).reshape(-1) for x in weights]
            for a, x in zip(sets, ws):
                if x.size != a.shape[0]:
                    raise ValueError(f"a set of {a.shape[0]} vectors needs {a.shape[0]} weights, got {x.size}")
                if not (np.isfinite(x).all() and (x >= 0).all()):
                    raise ValueError("weights must be finite and >= 0")
            w = np.concatenate(ws) if ws else np.zeros(0, np.float64)
        empty = [([], [], [], [], []) for _ in range(B)]
        with _Read(self._rw):
            # (never the graph path, never the coalescer: one exact device call for all sets)
            if self._vector_count == 0 or B == 0:
                return empty
            dim = self._dim
            for a in sets:
                if a.shape[0] and a.shape[1] != dim:
                    raise ValueError(f"Dimension mismatch: query has {a.shape[1]} dims, store holds {dim}")
            Q, offs = _vdb.pack_query_sets(sets, dim)
            mask = self._range_mask(Q, filter_metadata)  # None: no filter; False: nothing to search
            if mask is False:
                return empty
            scores, idx, fused, hits = self._index.search_fused(Q, offs, k, fetch_k, fusion, w, c, row_mask=mask,
                                                                with_fused=True, with_hits=True)
            meta = self._metadata
            out = []
            for b in range(B):
                valid = idx[b] >= 0
                ib = idx[b][valid].tolist()
                out.append((ib, scores[b][valid].astype(np.float64).tolist(),
                            [meta[i] if i < len(meta) else {} for i in ib], fused[b][valid].tolist(),
                            hits[b][valid].tolist()))
            return out

    # ---- sparse and hybrid query ----------------------------------------------------------
    def _attach_sparse(self, sparse_key: str) -> int:
        """Make the rows' sparse vectors under the metadata key ``sparse_key`` the sparse column
        attached to the index (read lock and _sparse_lock held) -> its ``n_terms`` (0: no row has an
        entry, nothing is searched).  Built once and kept under ``_attach_groups``' tag rule: while
        the key, the row count and the rows' contents stay as they were and the index still holds it
        (an add, a delete and a clear drop it; an upsert may change a row's metadata)."""
        n = self._vector_count
        tag = (sparse_key, n, self._index.stat("rows_updated"))
        if self._sparse_tag == tag and self._index.stat("sparse_rows") == n \
                and self._index.stat("sparse_sets") == self._sparse_sets:
            return self._sparse_terms
        indptr, terms, weights, n_terms = build_sparse_column(self._metadata, n, sparse_key)
        self._sparse_tag = None
        if n_terms == 0:  # no row has an entry: no other key's column stays attached
            if self._index.stat("sparse_rows"):
                self._index.set_sparse(None)
        else:
            self._index.set_sparse(indptr, terms, weights, n_terms)
            self._sparse_tag, self._sparse_terms = tag, n_terms
            self._sparse_sets = self._index.stat("sparse_sets")
        return n_terms

    def sparse_query(self, sparse, k: int = 10, filter_metadata: Optional[Dict] = None,
                     sparse_key: str = "sparse") -> Tuple:
        """The ``k`` rows whose sparse vector (metadata key ``sparse_key``: ``{"indices": [...],
        "values": [...]}``, e.g. BM25, SPLADE or BGE-M3 term weights) has the greatest dot product
        with ``sparse`` (the same form) -> (indices, scores, metadata), best first; only rows that
        share a term with the query are returned, ties go to the lower row id.  Exact, in fp64, on the
        device (include/vdb.h vdb_index_search_sparse).  The reference has no such read."""
        return self.batch_sparse_query([sparse], k, filter_metadata, sparse_key)[0]

    def batch_sparse_query(self, sparses, k: int = 10, filter_metadata: Optional[Dict] = None,
                           sparse_key: str = "sparse") -> List[Tuple]:
        """``sparse_query`` for a list of sparse vectors from one device call: one (indices, scores,
        metadata) tuple per query."""
        if len(self._devices()) > 1:
            raise NotImplementedError("sparse query is not supported on a multi-device store")
        k = int(k)
        if not 1 <= k <= SPARSE_MAX_K:
            raise ValueError(f"k must be in [1, {SPARSE_MAX_K}], got {k}")
        qs = [normalize_sparse_query(s) for s in sparses]
        B = len(qs)
        empty = [([], [], []) for _ in range(B)]
        with _Read(self._rw):
            if self._vector_count == 0 or B == 0:
                return empty
            mask = self._sparse_mask(filter_metadata)
            if mask is False:
                return empty
            with self._sparse_lock:  # one attached column: attach and search as one step
                n_terms = self._attach_sparse(sparse_key)
                if n_terms == 0:
                    return empty
                ip, t, w = _vdb.pack_sparse_vectors([clip_sparse_query(q, n_terms) for q in qs])
                scores, idx = self._index.search_sparse(ip, t, w, k, row_mask=mask)
            meta = self._metadata
            out = []
            for b in range(B):
                valid = idx[b] >= 0
                ib = idx[b][valid].tolist()
                out.append((ib, scores[b][valid].astype(np.float64).tolist(), [meta[i] if i < len(meta) else {} for i in ib]))
            return out

    def _sparse_mask(self, filter_metadata: Optional[Dict]):
        """The row_mask of a sparse read (read lock held, rows present): None without a filter, False
        when nothing matches the filter (no device call is needed)."""
        if not filter_metadata:
            return None
        mask, eligible = self._filter_masks([filter_metadata], self._vector_count)[0]
        return mask if eligible else False

    def hybrid_query(self, query_vector: Union[np.ndarray, Any], sparse, k: int = 10, fetch_k: Optional[int] = None,
                     weights=(1.0, 1.0), rrf_c: float = 60.0, filter_metadata: Optional[Dict] = None,
                     sparse_key: str = "sparse") -> Tuple:
        """Dense and sparse retrieval fused: the best ``fetch_k`` rows (``None``: min(200, max(k, 4
        k))) of ``query`` for ``query_vector`` and the best ``fetch_k`` of ``sparse_query`` for
        ``sparse`` are fused per row by weighted reciprocal rank, ``weights[0] / (rrf_c + dense rank) +
        weights[1] / (rrf_c + sparse rank)``, -> (indices, scores, metadata, fused, hits) as
        ``fused_query`` returns them (hits: 1 or 2).  Ties go to the lower row id.  One device call,
        exact and the same for every precision (include/vdb.h vdb_index_search_hybrid)."""
        q = _as_matrix(query_vector)
        if q.ndim == 2 and q.shape[0] == 1:
            q = q[0]
        if q.ndim != 1:
            raise ValueError(f"hybrid_query takes one vector of shape (dim,) or (1, dim), got {q.shape}; "
                             "use batch_hybrid_query for several")
        return self.batch_hybrid_query(q[None, :], [sparse], k, fetch_k, weights, rrf_c, filter_metadata, sparse_key)[0]

    def batch_hybrid_query(self, query_vectors: Union[np.ndarray, Any], sparses, k: int = 10,
                           fetch_k: Optional[int] = None, weights=(1.0, 1.0), rrf_c: float = 60.0,
                           filter_metadata: Optional[Dict] = None, sparse_key: str = "sparse") -> List[Tuple]:
        """``hybrid_query`` for a [B, dim] block of vectors and B sparse vectors from one device call:
        one (indices, scores, metadata, fused, hits) tuple per query."""
        if len(self._devices()) > 1:
            raise NotImplementedError("hybrid query is not supported on a multi-device store")
        k = int(k)
        if not 1 <= k <= FUSED_MAX_K:
            raise ValueError(f"k must be in [1, {FUSED_MAX_K}], got {k}")
        fetch_k = min(FUSED_MAX_FETCH, max(k, 4 * k)) if fetch_k is None else int(fetch_k)
        if not k <= fetch_k <= FUSED_MAX_FETCH:
            raise ValueError(f"fetch_k must be in [k, {FUSED_MAX_FETCH}], got fetch_k={fetch_k} k={k}")
        c = float(rrf_c)
        if not 0.0 <= c < float("inf"):  # (a NaN fails both comparisons)
            raise ValueError(f"rrf_c must be finite and >= 0, got {rrf_c}")
        w = np.asarray(weights, dtype=np.float64).reshape(-1)
        if w.size != 2 or not (np.isfinite(w).all() and (w >= 0).all()):
            raise ValueError("weights must be (w_dense, w_sparse), finite and >= 0")
        Q = _as_matrix(query_vectors)
        if Q.ndim == 1:
            Q = Q[None, :]
        if Q.ndim != 2:
            raise ValueError(f"query_vectors must be 2-D (B, dim), got {Q.shape}")
        qs = [normalize_sparse_query(s) for s in sparses]
        B = Q.shape[0]
        if len(qs) != B:
            raise ValueError(f"{B} query vectors need {B} sparse vectors, got {len(qs)}")
        empty = [([], [], [], [], []) for _ in range(B)]
        with _Read(self._rw):
            # (never the graph path, never the coalescer: one exact device call for the block)
            mask = self._range_mask(Q, filter_metadata)  # None: no filter; False: nothing to search
            if mask is False or B == 0:
                return empty
            with self._sparse_lock:  # one attached column: attach and search as one step
                n_terms = self._attach_sparse(sparse_key)
                if n_terms == 0:  # no row has a sparse entry: an empty column of one term, every sparse list empty
                    self._index.set_sparse(np.zeros(self._vector_count + 1, np.int64), None, None, 1)
                    n_terms = 1
                ip, t, sw = _vdb.pack_sparse_vectors([clip_sparse_query(q, n_terms) for q in qs])
                scores, idx, fused, hits = self._index.search_hybrid(Q, ip, t, sw, k, fetch_k, (float(w[0]), float(w[1])),
                                                                     c, row_mask=mask, with_fused=True, with_hits=True)
            meta = self._metadata
            out = []
            for b in range(B):
                valid = idx[b] >= 0
                ib = idx[b][valid].tolist()
                out.append((ib, scores[b][valid].astype(np.float64).tolist(),
                            [meta[i] if i < len(meta) else {} for i in ib], fused[b][valid].tolist(),
                            hits[b][valid].tolist()))
            return out

    def hybrid_sum_query(self, query_vector: Union[np.ndarray, Any], sparse, k: int = 10, weights=(1.0, 1.0),
                         filter_metadata: Optional[Dict] = None, sparse_key: str = "sparse") -> Tuple:
        """Dense and sparse retrieval combined by a weighted sum of the two SCORES: every row is ranked
        by ``weights[0] * dense + weights[1] * sparse``, ``dense`` its exact key for ``query_vector``
        (the cosine similarity; minus the SQUARED distance for euclidean) and ``sparse`` the dot product
        of its sparse vector (metadata key ``sparse_key``) with ``sparse``, 0 for a row that shares no
        term -> (indices, scores, metadata, dense, sparse), best first; ties go to the lower row id.
        Unlike ``hybrid_query`` (reciprocal rank of two fetched lists) the score magnitudes count and
        nothing is fetched first: the sum is formed for every row of the store, in fp64, so a row that
        is far down both rankings and still has the best sum is found.  Every row is a candidate,
        whether it shares a term or not.  Pinecone's sparse-dense ``alpha`` is ``weights=(alpha, 1 -
        alpha)``; Milvus' WeightedRanker and Elasticsearch's linear retriever are the same sum.  The
        weights lie in [0, 2^64]; scores are not normalised.  One device call, exact and the same for
        every precision (include/vdb.h vdb_index_search_hybrid_sum).  The reference has no such
        read."""
        q = _as_matrix(query_vector)
        if q.ndim == 2 and q.shape[0] == 1:
            q = q[0]
        if q.ndim != 1:
            raise ValueError(f"hybrid_sum_query takes one vector of shape (dim,) or (1, dim), got {q.shape}; "
                             "use batch_hybrid_sum_query for several")
        return self.batch_hybrid_sum_query(q[None, :], [sparse], k, weights, filter_metadata, sparse_key)[0]

    def batch_hybrid_sum_query(self, query_vectors: Union[np.ndarray, Any], sparses, k: int = 10, weights=(1.0, 1.0),
                               filter_metadata: Optional[Dict] = None, sparse_key: str = "sparse") -> List[Tuple]:
        """``hybrid_sum_query`` for a [B, dim] block of vectors and B sparse vectors from one device
        call: one (indices, scores, metadata, dense, sparse) tuple per query."""
        if len(self._devices()) > 1:
            raise NotImplementedError("hybrid sum query is not supported on a multi-device store")
        k = int(k)
        if not 1 <= k <= HYBRID_SUM_MAX_K:
            raise ValueError(f"k must be in [1, {HYBRID_SUM_MAX_K}], got {k}")
        w = np.asarray(weights, dtype=np.float64).reshape(-1)
        if w.size != 2 or not ((w >= 0).all() and (w <= HYBRID_SUM_MAX_WEIGHT).all()):  # (a NaN fails both)
            raise ValueError("weights must be (w_dense, w_sparse), each in [0, 2^64]")
        Q = _as_matrix(query_vectors)
        if Q.ndim == 1:
            Q = Q[None, :]
        if Q.ndim != 2:
            raise ValueError(f"query_vectors must be 2-D (B, dim), got {Q.shape}")
        qs = [normalize_sparse_query(s) for s in sparses]
        B = Q.shape[0]
        if len(qs) != B:
            raise ValueError(f"{B} query vectors need {B} sparse vectors, got {len(qs)}")
        if B > HYBRID_SUM_MAX_QUERIES:
            raise ValueError(f"at most {HYBRID_SUM_MAX_QUERIES} queries per call, got {B}")
        empty = [([], [], [], [], []) for _ in range(B)]
        with _Read(self._rw):
            # (never the graph path, never the coalescer: one exact device call for the block)
            mask = self._range_mask(Q, filter_metadata)  # None: no filter; False: nothing to search
            if mask is False or B == 0:
                return empty
            with self._sparse_lock:  # one attached column: attach and search as one step
                n_terms = self._attach_sparse(sparse_key)
                if n_terms == 0:  # no row has a sparse entry: an empty column of one term, every sparse key 0
                    self._index.set_sparse(np.zeros(self._vector_count + 1, np.int64), None, None, 1)
                    n_terms = 1
                ip, t, sw = _vdb.pack_sparse_vectors([clip_sparse_query(q, n_terms) for q in qs])
                scores, idx, dense, sparse = self._index.search_hybrid_sum(Q, ip, t, sw, k, (float(w[0]), float(w[1])),
                                                                           row_mask=mask, with_parts=True)
            meta = self._metadata
            out = []
            for b in range(B):
                valid = idx[b] >= 0
                ib = idx[b][valid].tolist()
                out.append((ib, scores[b][valid].astype(np.float64).tolist(),
                            [meta[i] if i < len(meta) else {} for i in ib], dense[b][valid].tolist(),
                            sparse[b][valid].tolist()))
            return out

    # ---- MaxSim query ------------------------------------------------------------------
    def maxsim_query(self, query_vectors: Union[np.ndarray, Any], group_by: str, k: int = 10,
                     filter_metadata: Optional[Dict] = None) -> List[Dict]:
        """Late-interaction ("MaxSim": ColBERT / ColPali token embeddings) retrieval: the ``k`` best
        values of the metadata key ``group_by`` for a set of query vectors [T, dim], T <= 64 -> a
        list of ``{"group": value, "score": float, "sum": float}``, best first.  A group's sum is,
        over the query vectors, the vector's best exact key among the group's rows (cosine
        similarity; minus the SQUARED distance for euclidean), added in vector order in fp64;
        ``score`` is that sum rounded to fp32.  Ties go to the group seen first in the store; rows
        without the key belong to no group.  Exact over the whole corpus and the same for every
        precision (include/vdb.h vdb_index_search_maxsim).  The reference has no such read."""
        q = _as_matrix(query_vectors)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2:
            raise ValueError(f"maxsim_query takes one set of vectors of shape (T, dim), got {q.shape}; "
                             "use batch_maxsim_query for several sets")
        return self.batch_maxsim_query([q], group_by, k, filter_metadata)[0]

    def batch_maxsim_query(self, query_sets, group_by: str, k: int = 10,
                           filter_metadata: Optional[Dict] = None) -> List[List[Dict]]:
        """``maxsim_query`` for a list of query sets from one device call: one list of groups per
        set."""
        if len(self._devices()) > 1:
            raise NotImplementedError("MaxSim query is not supported on a multi-device store")
        k = int(k)
        if not 1 <= k <= MAXSIM_MAX_K:
            raise ValueError(f"k must be in [1, {MAXSIM_MAX_K}], got {k}")
        sets = []
        for s in query_sets:
            a = _as_matrix(s)
            if a.size == 0:  # a set without a vector: no error, no result
                a = np.zeros((0, 0), np.float32)
            elif a.ndim == 1:
                a = a[None, :]
            if a.ndim != 2:
                raise ValueError(f"a query set must be 2-D (T, dim), got {a.shape}")
            if a.shape[0] > MAXSIM_MAX_VECTORS:
                raise ValueError(f"a query set takes at most {MAXSIM_MAX_VECTORS} vectors, got {a.shape[0]}")
            sets.append(a)
        B = len(sets)
        empty = [[] for _ in range(B)]
        with _Read(self._rw):
            # (never the graph path, never the coalescer: one exact device call for all sets)
            if self._vector_count == 0 or B == 0:
                return empty
            dim = self._dim
            for a in sets:
                if a.shape[0] and a.shape[1] != dim:
                    raise ValueError(f"Dimension mismatch: query has {a.shape[1]} dims, store holds {dim}")
            Q, offs = _vdb.pack_query_sets(sets, dim)
            mask = self._range_mask(Q, filter_metadata)  # None: no filter; False: nothing to search
            if mask is False:
                return empty
            with self._group_lock:  # one attached column: attach and search as one step
                values = self._attach_groups(group_by)
                if not values:  # no row has the key
                    return empty
                if Q.shape[0] and len(values) > MAXSIM_MAX_CELLS // Q.shape[0]:
                    raise ValueError(f"{Q.shape[0]} query vectors x {len(values)} groups pass the "
                                     f"{MAXSIM_MAX_CELLS} table entries of one call; send fewer sets at a time")
                scores, grp, sums = self._index.search_maxsim((Q, offs), len(values), k, row_mask=mask, with_sums=True)
            return [[{"group": values[g], "score": float(sc), "sum": float(sm)}
                     for g, sc, sm in zip(grp[b][grp[b] >= 0].tolist(), scores[b][grp[b] >= 0].tolist(),
                                          sums[b][grp[b] >= 0].tolist())] for b in range(B)]

    # ---- recommend --------------------------------------------------------------------
    def recommend(self, positive, negative=None, k: int = 10, filter_metadata: Optional[Dict] = None,
                  key: Optional[Any] = None) -> Tuple:
        """The ``k`` rows most like the stored examples ``positive`` and unlike ``negative`` ->
        (indices, scores, metadata) as ``query`` returns them, best first, the examples themselves
        left out.  With ``key=None`` the entries are row indices; with a metadata field (``key=
        "doc_id"``) each entry is a value and every row that holds it becomes an example ("more
        like this document" = all its chunks).  The query is built on the device, the mean of the
        positives, or ``2 * mean(positive) - mean(negative)`` (for cosine over the normalised
        rows), in one fixed fp64 order, so the answer is exact and the same for every precision
        (include/vdb.h vdb_index_search_recommend).  At most 64 examples and ``k`` <= 136.  The
        reference has no such read."""
        return self.batch_recommend([(positive, negative)], k, filter_metadata, key)[0]

    def batch_recommend(self, requests, k: int = 10, filter_metadata: Optional[Dict] = None,
                        key: Optional[Any] = None) -> List[Tuple]:
        """``recommend`` for a list of ``(positive, negative)`` pairs from one device call: one
        (indices, scores, metadata) tuple per pair."""
        if len(self._devices()) > 1:
            raise NotImplementedError("recommend is not supported on a multi-device store")
        k = int(k)
        if not 1 <= k <= REC_MAX_K:
            raise ValueError(f"k must be in [1, {REC_MAX_K}], got {k}")
        requests = [(r[0], r[1] if len(r) > 1 else None) for r in requests]
        B = len(requests)
        with _Read(self._rw):
            # (never the graph path, never the coalescer: one exact device call for the block)
            n = self._vector_count
            pos = [self._example_rows(p, key, n) for p, _ in requests]
            neg = [self._example_rows(g, key, n) for _, g in requests]
            for p, g in zip(pos, neg):
                if p.size + g.size > REC_MAX_EXAMPLES:
                    raise ValueError(f"a recommend query takes at most {REC_MAX_EXAMPLES} examples, positives and "
                                     f"negatives together; got {p.size + g.size}")
            empty = [([], [], []) for _ in range(B)]
            if n == 0 or not any(p.size for p in pos):
                return empty
            if not self._compiled_similarity_fn:
                raise RuntimeError(_NO_OPERATOR_MSG)
            mask = None
            if filter_metadata:
                mask, eligible = self._filter_masks([filter_metadata], n)[0]
                if not eligible:
                    return empty
            scores, idx = self._index.search_recommend(pos, neg if any(g.size for g in neg) else None, k, row_mask=mask)
            meta = self._metadata
            out = []
            for b in range(B):
                valid = idx[b] >= 0
                ib = idx[b][valid].tolist()
                out.append((ib, scores[b][valid].astype(np.float64).tolist(),
                            [meta[i] if i < len(meta) else {} for i in ib]))
            return out

    def _example_rows(self, entries, key, n: int) -> np.ndarray:
        """The row ids of one example list (read lock held): the entries themselves (``key`` None:
        integers in [0, n)), or every row whose metadata holds ``key`` with an entry's value."""
        if entries is None:
            return np.zeros(0, np.int64)
        entries = list(entries)
        if key is None:
            for e in entries:
                if isinstance(e, (bool, np.bool_)) or not isinstance(e, (int, np.integer)):
                    raise ValueError(f"an example must be an integer row index (or pass key=), got {e!r}")
                if not 0 <= int(e) < n:
                    raise ValueError(f"row index {int(e)} is outside [0, {n})")
            return np.asarray([int(e) for e in entries], np.int64).reshape(-1)
        rows = []
        for v in entries:
            r = self._meta_index.rows_with(key, v)
            r = r[r < n]
            if r.size == 0:
                raise ValueError(f"no row has {key!r} = {v!r}")
            rows.append(r)
        return np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)

    # ---- misc API ----------------------------------------------------------------------
    def _warmup_kernels(self):
        """service/optimized_vector_store.py:194-196 (a no-op there); here: one tiny search."""
        if self._vector_count and self._compiled_similarity_fn:
            self._index.search(np.zeros((1, self._dim), np.float32) + 1.0, 1)

    def clear(self):
        """service/optimized_vector_store.py:198-209."""
        with self._lock, _Write(self._rw):
            try:
                if self.store_path.exists():
                    shutil.rmtree(self.store_path)
                self.store_path.mkdir(parents=True, exist_ok=True)
                self._files = StoreFiles(self.store_path)
                self._create_empty_store()
                if self.config.enable_hnsw:  # :205-206
                    from performance.hnsw_index import ProductionHNSWIndex
                    self._hnsw_index = ProductionHNSWIndex(self.config.dimension, self.store_path,
                                                           self.config.metric, device=self._devices()[0])
            except Exception as e:  # the reference logs and swallows (:208-209)
                logger.error("clearing store %s failed: %s", self.store_path, e)

    def optimize(self) -> Dict[str, Any]:
        """Callers: api/routes/admin.py:230, api/routes/performance.py:188, tests/demo.py:248.
        Flushes persistence and pre-sizes the device corpus to a 256-row multiple."""
        t0 = time.time()
        with self._lock, _Write(self._rw):
            if self._index is not None:
                self._index.reserve(self._vector_count)
            self._is_dirty = True
            self._save_store(force=True)
        with _Read(self._rw):
            self._warmup_kernels()
        return {"optimized": True, "vector_count": self._vector_count,
                "optimization_time_ms": (time.time() - t0) * 1000.0}

    def health_check(self) -> Dict[str, Any]:
        """Caller: tests/demo.py:254 (reads 'healthy' and 'issues')."""
        issues = []
        if len(self._metadata) != self._vector_count:
            issues.append(f"metadata rows ({len(self._metadata)}) != vectors ({self._vector_count})")
        if self._vector_count and self._index is None:
            issues.append("device index missing")
        if self._index is not None and self._index.count() != self._vector_count:
            issues.append("device row count out of sync")
        if not self._compiled_similarity_fn:
            issues.append(_NO_OPERATOR_MSG)
        return {"healthy": not issues, "issues": issues, "vector_count": self._vector_count,
                "metric": self.config.metric, "devices": self._devices()}

    def get_stats(self):
        """service/optimized_vector_store.py:241-242 (+ memory_usage_mb, read by
        api/routes/monitoring.py:153 and tests/demo.py:146)."""
        mem = 0.0
        if self._index is not None:
            mem = self._index.stat("device_bytes") / (1024.0 * 1024.0)
        return {"vector_count": self._vector_count, "dimension": self.config.dimension,
                "metric": self.config.metric,
                "index_type": "hnsw" if self.config.enable_hnsw else "flat",
                "memory_usage_mb": mem}

    # ---- persistence: vectors.npz + metadata.jsonl (service/optimized_vector_store.py:218-239)
    # plus an append log between compactions (service/persistence.py)
    def _save_store(self, force: bool = False):
        """Compaction: the whole store as the reference's two files (log dropped)."""
        if not (self.config.persist or force):
            return
        if self._vector_count == 0 or not (self._is_dirty or self._files.log_rows):
            return
        self._files.compact(self._index.get_vectors(), self._metadata[: self._vector_count])
        self._is_dirty = False

    def _load_store(self):
        try:
            vecs, meta = self._files.load()
            if vecs.shape[0] == 0:
                self._create_empty_store()
                return
            self._ensure_index(vecs.shape[1]).add(vecs)
            self._metadata = meta
            self._meta_index.clear()
            self._meta_index.extend(meta)
            self._vector_count = self._index.count()
            if self._hnsw_index is not None:
                if not self._hnsw_index.attach(self._index):
                    self._hnsw_index.build(None, native_index=self._index)
        except Exception as e:  # reference: log and start empty (:237-239)
            logger.error("loading store %s failed, starting empty: %s", self.store_path, e)
            self._create_empty_store()


def create_optimized_vector_store(store_path: str, dimension: int = 384, jit_compile: bool = True,
                                  enable_hnsw: bool = False, **kwargs) -> MLXVectorStore:
    """service/optimized_vector_store.py:244-246."""
    config = MLXVectorStoreConfig(dimension=dimension, jit_compile=jit_compile, enable_hnsw=enable_hnsw, **kwargs)
    return MLXVectorStore(store_path, config)


# ---- functional API (tests/test_vector_store.py:15-43 imports these) -----------------------
_STORES: Dict[str, MLXVectorStore] = {}
_STORES_LOCK = threading.Lock()


def _base_dir() -> Path:
    # the REST manager's layout, api/routes/vectors.py:57
    return Path(os.environ.get("VECTOR_STORE_BASE", "~/.team_mind_data/vector_stores")).expanduser()


def _store_path(user_id: str, model_id: str) -> Path:
    return _base_dir() / user_id / model_id


def _key(user_id: str, model_id: str) -> str:
    return f"{user_id}_{model_id}"  # api/routes/vectors.py:45-46


def store_exists(user_id: str, model_id: str) -> bool:
    return _key(user_id, model_id) in _STORES or _store_path(user_id, model_id).exists()


def create_store(user_id: str, model_id: str, dimension: int = 384, metric: str = "cosine",
                 **kwargs) -> MLXVectorStore:
    with _STORES_LOCK:
        key = _key(user_id, model_id)
        if key not in _STORES:
            cfg = MLXVectorStoreConfig(dimension=dimension, metric=metric, **kwargs)
            _STORES[key] = MLXVectorStore(str(_store_path(user_id, model_id)), cfg)
        return _STORES[key]


def _get_store(user_id: str, model_id: str) -> MLXVectorStore:
    key = _key(user_id, model_id)
    if key not in _STORES:
        return create_store(user_id, model_id)  # lazy creation, api/routes/vectors.py:53-69
    return _STORES[key]


def add_vectors(user_id: str, model_id: str, vectors, metadata: List[Dict]) -> Dict[str, int]:
    return _get_store(user_id, model_id).add_vectors(vectors, metadata)


def upsert_vectors(user_id: str, model_id: str, vectors, metadata: List[Dict], key: str = "id") -> Dict[str, int]:
    return _get_store(user_id, model_id).upsert_vectors(vectors, metadata, key=key)


def query_vectors(user_id: str, model_id: str, query_vector, k: int = 10,
                  filter_metadata: Optional[Dict] = None) -> List[Dict[str, Any]]:
    """-> [{"index", "score", "metadata"}] (service/models.py SearchResult shape)."""
    idx, scores, meta = _get_store(user_id, model_id).query(query_vector, k=k, filter_metadata=filter_metadata)
    return [{"index": i, "score": s, "metadata": m} for i, s, m in zip(idx, scores, meta)]


def count_vectors(user_id: str, model_id: str) -> Dict[str, int]:
    st = _get_store(user_id, model_id)
    return {"vectors": st._vector_count, "metadata": len(st._metadata)}


def delete_store(user_id: str, model_id: str) -> bool:
    with _STORES_LOCK:
        st = _STORES.pop(_key(user_id, model_id), None)
    path = _store_path(user_id, model_id)
    if st is not None and st._index is not None:
        st._index.close()
    if path.exists():
        shutil.rmtree(path)
        return True
    return st is not None
