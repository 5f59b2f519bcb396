"""ctypes binding of the gfx950 vector-search core (include/vdb.h, lib/libvdb_amd.so).

This is the only way the store reaches the device.  There is no CPU fallback:
if the shared library is missing, or no gfx950 device is visible, every
constructor here raises.  (The CPU oracle under ``oracle/`` is test
infrastructure and is never imported by this package.)
"""
from __future__ import annotations

import ctypes
import os
import threading
from pathlib import Path
from typing import Optional, Tuple

import numpy as np

_PKG_ROOT = Path(__file__).resolve().parent.parent
_DEFAULT_LIB = _PKG_ROOT / "lib" / "libvdb_amd.so"

VDB_OK = 0
VDB_ERR_INVALID = -1
VDB_ERR_HIP = -2
VDB_ERR_OOM = -3
VDB_ERR_NONFINITE = -4
VDB_ERR_UNSUPPORTED = -5
VDB_ERR_NODEVICE = -6

METRIC_IDS = {"cosine": 0, "euclidean": 1}
# candidate-pass arithmetic (include/vdb.h VDB_PREC_*); results are identical, speed differs
PRECISION_IDS = {"fp32": 0, "bf16x3": 1, "bf16": 2, "auto": 3, "i8": 4, "i8x3": 5, "i8q": 6}
MEM_HOST = 0
MEM_DEVICE = 1
# largest beam (ef) vdb_graph_search accepts (csrc/vdb_graph.hip GS_EF_MAX)
GRAPH_EF_MAX = 256
# how vdb_index_search_fused combines a set's lists (include/vdb.h VDB_FUSE_*)
FUSION_IDS = {"rrf": 0, "max": 1}
# largest k vdb_index_search_hybrid_sum accepts (csrc/vdb_hybsum_plan.h kHybsumMaxK)
HYBRID_SUM_MAX_K = 1024
# vdb_index_set_column / vdb_index_filter_mask (include/vdb.h VDB_FILTER_*, csrc/vdb_filter_plan.h)
FILTER_LO_INCL = 1
FILTER_HI_INCL = 2
FILTER_NEGATE = 4
FILTER_SLOTS = 16
FILTER_MAX_PREDS = 256
FILTER_MAX_CLAUSES = 8
# the layout of vdb_filter_clause: int32 column, int32 flags, fp64 lo, fp64 hi (24 bytes)
FILTER_CLAUSE_DTYPE = np.dtype([("column", "<i4"), ("flags", "<i4"), ("lo", "<f8"), ("hi", "<f8")])

# Every symbol include/vdb.h declares (tests/test_abi.py checks the .so exports them).
EXPORTED_SYMBOLS = (
    "vdb_last_error", "vdb_version", "vdb_device_count",
    "vdb_index_create", "vdb_index_destroy", "vdb_index_reserve",
    "vdb_index_set_param", "vdb_index_get_stat",
    "vdb_index_add", "vdb_index_count", "vdb_index_clear", "vdb_index_remove", "vdb_index_update",
    "vdb_index_get_vectors",
    "vdb_index_search", "vdb_index_search_rows", "vdb_index_search_range",
    "vdb_index_set_column", "vdb_index_filter_mask",
    "vdb_index_set_groups", "vdb_index_search_groups", "vdb_index_search_mmr", "vdb_index_search_recommend", "vdb_index_search_fused", "vdb_index_search_maxsim",
    "vdb_index_set_sparse", "vdb_index_search_sparse", "vdb_index_search_hybrid", "vdb_index_search_hybrid_sum", "vdb_merge_topk", "vdb_similarity_matrix", "vdb_normalize_rows", "vdb_topk_scores",
    "vdb_graph_build", "vdb_graph_import", "vdb_graph_export", "vdb_graph_add", "vdb_graph_info", "vdb_graph_search",
    "vdb_graph_stat", "vdb_graph_set_param", "vdb_graph_destroy",
    "vdb_shards_create", "vdb_shards_destroy", "vdb_shards_add", "vdb_shards_count", "vdb_shards_shard_count",
    "vdb_shards_search", "vdb_shards_search_device", "vdb_shards_get_vectors", "vdb_shards_clear", "vdb_shards_reserve",
    "vdb_shards_set_param", "vdb_shards_get_stat", "vdb_shutdown",
)

_lib = None
_lib_lock = threading.Lock()


class VDBError(RuntimeError):
    """A failing vdb_* call (HIP error, out of memory, no device)."""


def library_path() -> Path:
    return Path(os.environ.get("VDB_LIB", str(_DEFAULT_LIB)))


def _prefer_torch_runtime() -> None:
    # torch bundles its own libamdhip64.so.7; load it first so the process has
    # one HIP runtime whichever of torch / this library is imported first.
    try:  # pragma: no cover - depends on the environment
        import torch  # noqa: F401
    except Exception:
        pass


def load_library():
    """Load (once) and type the C-ABI.  Raises ImportError if it is not built."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        path = library_path()
        if not path.exists():
            raise ImportError(
                f"vdb HIP library not found at {path}; build it with "
                f"`make -C {_PKG_ROOT}` (hipcc --offload-arch=gfx950)")
        _prefer_torch_runtime()
        lib = ctypes.CDLL(str(path))
        c_i32, c_i64, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
        p_i64 = ctypes.POINTER(ctypes.c_int64)
        sig = {
            "vdb_last_error": (ctypes.c_char_p, []),
            "vdb_version": (c_i32, []),
            "vdb_device_count": (c_i32, [ctypes.POINTER(ctypes.c_int32)]),
            "vdb_index_create": (c_i32, [c_i32, c_i32, c_i32, ctypes.POINTER(c_vp)]),
            "vdb_index_destroy": (c_i32, [c_vp]),
            "vdb_index_reserve": (c_i32, [c_vp, c_i64]),
            "vdb_index_set_param": (c_i32, [c_vp, ctypes.c_char_p, c_i64]),
            "vdb_index_get_stat": (c_i32, [c_vp, ctypes.c_char_p, p_i64]),
            "vdb_index_add": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_vp]),
            "vdb_index_count": (c_i32, [c_vp, p_i64]),
            "vdb_index_clear": (c_i32, [c_vp]),
            "vdb_index_remove": (c_i32, [c_vp, c_vp, c_i32, c_vp, p_i64]),
            "vdb_index_update": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_i32, c_vp]),
            "vdb_index_get_vectors": (c_i32, [c_vp, c_i64, c_i64, c_vp]),
            "vdb_index_search": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_i64, c_vp]),
            "vdb_index_search_rows": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_vp, c_i32, c_vp, c_i64, c_vp, c_i32, c_vp, c_vp,
                                              c_vp, c_i64, c_vp]),
            "vdb_index_search_range": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64,
                                               c_vp]),
            "vdb_index_set_column": (c_i32, [c_vp, c_i32, c_vp, c_i64, c_i32, c_vp]),
            "vdb_index_filter_mask": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp]),
            "vdb_index_set_groups": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_vp]),
            "vdb_index_search_groups": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i64,
                                                c_vp]),
            "vdb_index_search_mmr": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, ctypes.c_double, c_vp, c_i32, c_vp, c_vp,
                                             c_vp, c_vp, c_i64, c_vp]),
            "vdb_index_search_recommend": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i32,
                                                   c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
            "vdb_index_search_fused": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_i32, c_i32,
                                               ctypes.c_double, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
            "vdb_index_search_maxsim": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_i32, c_i32, c_vp, c_i32, c_vp, c_vp,
                                                c_vp, c_vp]),
            "vdb_index_set_sparse": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_i32, c_i32, c_vp]),
            "vdb_index_search_sparse": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i64, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp,
                                                c_i64, c_vp]),
            "vdb_index_search_hybrid": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i64, c_i32, c_i32, ctypes.c_double,
                                                ctypes.c_double, ctypes.c_double, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp,
                                                c_i64, c_vp]),
            "vdb_index_search_hybrid_sum": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i64, c_i32, ctypes.c_double,
                                                    ctypes.c_double, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64,
                                                    c_vp]),
            "vdb_merge_topk": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
            "vdb_similarity_matrix": (c_i32, [c_vp, c_i64, c_i32, c_vp, c_i32, c_i32, c_vp, c_vp]),
            "vdb_normalize_rows": (c_i32, [c_vp, c_i64, c_i32, c_vp, c_vp]),
            "vdb_topk_scores": (c_i32, [c_vp, c_i32, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp]),
            "vdb_graph_build": (c_i32, [c_vp, c_i32, c_i32, c_i32, ctypes.POINTER(c_vp)]),
            "vdb_graph_import": (c_i32, [c_vp, c_i32, c_i64, c_vp, c_i32, c_vp, ctypes.POINTER(c_vp)]),
            "vdb_graph_export": (c_i32, [c_vp, c_vp, c_vp]),
            "vdb_graph_add": (c_i32, [c_vp]),
            "vdb_graph_info": (c_i32, [c_vp, p_i64, ctypes.POINTER(c_i32), ctypes.POINTER(c_i32)]),
            "vdb_graph_search": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
            "vdb_graph_stat": (c_i32, [c_vp, ctypes.c_char_p, p_i64]),
            "vdb_graph_set_param": (c_i32, [c_vp, ctypes.c_char_p, c_i64]),
            "vdb_graph_destroy": (c_i32, [c_vp]),
            "vdb_shards_create": (c_i32, [c_i32, c_i32, c_vp, c_i32, ctypes.POINTER(c_vp)]),
            "vdb_shards_destroy": (c_i32, [c_vp]),
            "vdb_shards_add": (c_i32, [c_vp, c_vp, c_i64]),
            "vdb_shards_count": (c_i32, [c_vp, p_i64]),
            "vdb_shards_shard_count": (c_i32, [c_vp, c_i32, p_i64]),
            "vdb_shards_search": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
            "vdb_shards_search_device": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
            "vdb_shards_get_vectors": (c_i32, [c_vp, c_i64, c_i64, c_vp]),
            "vdb_shards_clear": (c_i32, [c_vp]),
            "vdb_shards_reserve": (c_i32, [c_vp, c_i64]),
            "vdb_shards_set_param": (c_i32, [c_vp, ctypes.c_char_p, c_i64]),
            "vdb_shards_get_stat": (c_i32, [c_vp, ctypes.c_char_p, p_i64]),
            "vdb_shutdown": (c_i32, []),
        }
        for name, (res, args) in sig.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def _check(rc: int) -> None:
    if rc == VDB_OK:
        return
    msg = _lib.vdb_last_error().decode("utf-8", "replace")
    if rc in (VDB_ERR_INVALID, VDB_ERR_NONFINITE):
        raise ValueError(msg)
    raise VDBError(f"vdb error {rc}: {msg}")


def device_count() -> int:
    lib = load_library()
    n = ctypes.c_int32(0)
    lib.vdb_device_count(ctypes.byref(n))
    return int(n.value)


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def pack_predicates(predicates):
    """A list of lists of ``(slot, lo, hi, flags)`` -> (clauses FILTER_CLAUSE_DTYPE [n], offsets
    int32 [P + 1]): the arguments of vdb_index_filter_mask.  Nothing is validated here but the
    shape of a clause; the library checks the rest."""
    flat, offs = [], [0]
    for pred in predicates:
        for cl in pred:
            if len(cl) != 4:
                raise ValueError(f"a clause is (slot, lo, hi, flags), got {cl!r}")
            slot, lo, hi, flags = cl
            flat.append((int(slot), int(flags), float(lo), float(hi)))
        offs.append(len(flat))
    return np.array(flat, dtype=FILTER_CLAUSE_DTYPE).reshape(-1), np.asarray(offs, dtype=np.int32)


def rows_to_bitmap(mask_or_rows, count: int) -> np.ndarray:
    """The uint32 bitmap over ``count`` rows (bit r of word r/32 = row r) that
    vdb_index_remove takes, from a uint32 bitmap (checked for length) or from an integer array
    of row ids (ValueError when one is outside [0, count))."""
    a = np.asarray(mask_or_rows)
    need = (int(count) + 31) // 32
    if a.dtype == np.uint32:
        m = np.ascontiguousarray(a).reshape(-1)
        if m.size < need:
            raise ValueError(f"remove mask needs {need} uint32 words, got {m.size}")
        return m if m.size else np.zeros(1, np.uint32)
    if a.size and a.dtype.kind not in "iu":
        raise ValueError(f"row ids must be integers (or a uint32 bitmap), got dtype {a.dtype}")
    rows = a.astype(np.int64, copy=False).reshape(-1)
    if rows.size and (int(rows.min()) < 0 or int(rows.max()) >= count):
        raise ValueError(f"row ids must be in [0, {count}), got [{int(rows.min())}, {int(rows.max())}]")
    bits = np.zeros(max(need, 1) * 32, np.uint8)
    bits[rows] = 1
    return np.packbits(bits, bitorder="little").view(np.uint32)


def pack_query_sets(sets, dim: int) -> Tuple[np.ndarray, np.ndarray]:
    """A sequence of query sets, each [m, dim] (or one vector [dim]; m may be 0) -> what
    vdb_index_search_fused takes: the sub-queries back to back, fp32 [n_sub, dim], and the int64
    offsets [len(sets) + 1]."""
    arrs = []
    for a in sets:
        a = np.asarray(a, dtype=np.float32)
        if a.size == 0:
            a = a.reshape(0, dim)
        elif a.ndim == 1:
            a = a[None, :]
        if a.ndim != 2 or a.shape[1] != dim:
            raise ValueError(f"a query set must have shape (m, {dim}), got {a.shape}")
        arrs.append(a)
    offs = np.zeros(len(arrs) + 1, np.int64)
    if arrs:
        np.cumsum([a.shape[0] for a in arrs], out=offs[1:])
    q = np.concatenate(arrs) if arrs else np.zeros((0, dim), np.float32)
    return np.ascontiguousarray(q, dtype=np.float32), offs


def pack_sparse_vectors(vectors) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """A sequence of sparse vectors, each ``(indices, values)`` with the indices already strictly
    ascending (or ``None`` / an empty pair for a vector without entries) -> the CSR triple
    vdb_index_set_sparse and vdb_index_search_sparse take: int64 indptr [len + 1], int32 terms and
    fp32 weights back to back.  Nothing is sorted or checked here: the library validates."""
    ts, ws = [], []
    for v in vectors:
        if v is None:
            t, w = (), ()
        else:
            t, w = v
        t = np.asarray(t)
        if t.size and t.dtype.kind not in "iu":
            raise ValueError(f"term ids must be integers, got dtype {t.dtype}")
        if t.size and (int(t.min()) < -2**31 or int(t.max()) >= 2**31):
            raise ValueError("term ids must fit int32")
        w = np.asarray(w, dtype=np.float32).reshape(-1)
        t = t.astype(np.int32, copy=False).reshape(-1)
        if t.size != w.size:
            raise ValueError(f"a sparse vector needs one value per index, got {t.size} and {w.size}")
        ts.append(t)
        ws.append(w)
    indptr = np.zeros(len(ts) + 1, np.int64)
    if ts:
        np.cumsum([t.size for t in ts], out=indptr[1:])
    terms = np.concatenate(ts) if ts else np.zeros(0, np.int32)
    weights = np.concatenate(ws) if ws else np.zeros(0, np.float32)
    return indptr, np.ascontiguousarray(terms, np.int32), np.ascontiguousarray(weights, np.float32)


def pack_row_lists(lists) -> Tuple[np.ndarray, np.ndarray]:
    """A sequence of integer row-id arrays -> the CSR pair vdb_index_search_rows takes: int64
    offsets [len(lists) + 1] and the lists' ids back to back (int64)."""
    arrs = []
    for a in lists:
        a = np.asarray(a)
        if a.size and a.dtype.kind not in "iu":
            raise ValueError(f"row ids must be integers, got dtype {a.dtype}")
        arrs.append(a.astype(np.int64, copy=False).reshape(-1))
    offs = np.zeros(len(arrs) + 1, np.int64)
    if arrs:
        np.cumsum([a.size for a in arrs], out=offs[1:])
    rows = np.concatenate(arrs) if arrs else np.zeros(0, np.int64)
    return offs, np.ascontiguousarray(rows, dtype=np.int64)


class NativeIndex:
    """One device-resident corpus (tiled fp32 + norms) on one GPU."""

    def __init__(self, dim: int, metric: str = "cosine", device: int = 0, precision: Optional[str] = None):
        if metric not in METRIC_IDS:
            raise ValueError(f"unsupported metric {metric!r}; the vdb core implements {sorted(METRIC_IDS)}")
        self._lib = load_library()
        self.dim = int(dim)
        self.metric = metric
        self.device = int(device)
        h = ctypes.c_void_p()
        _check(self._lib.vdb_index_create(self.dim, METRIC_IDS[metric], self.device, ctypes.byref(h)))
        self._h = h
        if precision is not None:
            self.set_precision(precision)

    # -- lifecycle -------------------------------------------------------------
    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.vdb_index_destroy(h)

    def __del__(self):  # pragma: no cover - GC timing
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, rows: int) -> None:
        _check(self._lib.vdb_index_reserve(self._h, int(rows)))

    def set_param(self, name: str, value: int) -> None:
        _check(self._lib.vdb_index_set_param(self._h, name.encode(), int(value)))

    def set_precision(self, precision: str) -> None:
        if precision not in PRECISION_IDS:
            raise ValueError(f"precision must be one of {sorted(PRECISION_IDS)}, got {precision!r}")
        self.set_param("precision", PRECISION_IDS[precision])

    @property
    def precision(self) -> str:
        v = self.stat("precision")
        return next(k for k, i in PRECISION_IDS.items() if i == v)

    def stat(self, name: str) -> int:
        v = ctypes.c_int64(0)
        _check(self._lib.vdb_index_get_stat(self._h, name.encode(), ctypes.byref(v)))
        return int(v.value)

    # -- data ------------------------------------------------------------------
    def add(self, vectors: np.ndarray) -> None:
        v = np.ascontiguousarray(vectors, dtype=np.float32)
        if v.ndim != 2 or v.shape[1] != self.dim:
            raise ValueError(f"vectors must have shape (n, {self.dim}), got {v.shape}")
        if v.shape[0] == 0:
            return
        _check(self._lib.vdb_index_add(self._h, _ptr(v), v.shape[0], MEM_HOST, None))

    def add_device(self, ptr: int, n: int, stream: int = 0) -> None:
        _check(self._lib.vdb_index_add(self._h, ctypes.c_void_p(ptr), int(n), MEM_DEVICE, ctypes.c_void_p(stream)))

    def count(self) -> int:
        n = ctypes.c_int64(0)
        _check(self._lib.vdb_index_count(self._h, ctypes.byref(n)))
        return int(n.value)

    def clear(self) -> None:
        _check(self._lib.vdb_index_clear(self._h))

    def remove(self, mask_or_rows) -> int:
        """include/vdb.h vdb_index_remove: drop rows, the survivors keep their order and move
        down.  ``mask_or_rows``: a uint32 bitmap (ceil(count/32) words, bit r of word r/32 = row
        r removed) or an integer array of row ids (any order, repeats allowed).  Returns the
        number of rows removed.  An id outside [0, count) raises ValueError and changes nothing."""
        mask = rows_to_bitmap(mask_or_rows, self.count())
        n = ctypes.c_int64(0)
        _check(self._lib.vdb_index_remove(self._h, _ptr(mask), MEM_HOST, None, ctypes.byref(n)))
        return int(n.value)

    def remove_device(self, mask_ptr: int, stream: int = 0) -> int:
        """vdb_index_remove with a device-memory bitmap, read after the work queued on ``stream``."""
        n = ctypes.c_int64(0)
        _check(self._lib.vdb_index_remove(self._h, ctypes.c_void_p(mask_ptr or None), MEM_DEVICE,
                                          ctypes.c_void_p(stream or None), ctypes.byref(n)))
        return int(n.value)

    def update(self, rows, vectors: np.ndarray) -> int:
        """include/vdb.h vdb_index_update: row rows[i] becomes vectors[i], in place.  ``rows``:
        integer row ids (any integer dtype, any order, pairwise distinct); ``vectors``: shape
        (len(rows), dim).  Returns the number of rows updated.  An id outside [0, count), a
        repeated id or a non-finite value raises ValueError and changes nothing."""
        r = np.asarray(rows)
        if r.size and r.dtype.kind not in "iu":
            raise ValueError(f"row ids must be integers, got dtype {r.dtype}")
        r = np.ascontiguousarray(r.reshape(-1), dtype=np.int64)
        v = np.ascontiguousarray(vectors, dtype=np.float32)
        if v.ndim != 2 or v.shape != (r.size, self.dim):
            raise ValueError(f"vectors must have shape ({r.size}, {self.dim}), got {v.shape}")
        if r.size == 0:
            return 0
        _check(self._lib.vdb_index_update(self._h, _ptr(r), _ptr(v), r.size, MEM_HOST, None))
        return int(r.size)

    def update_device(self, rows_ptr: int, vectors_ptr: int, n: int, stream: int = 0) -> int:
        """vdb_index_update with device-memory arguments (int64 ids and fp32 rows), read after the
        work queued on ``stream``."""
        _check(self._lib.vdb_index_update(self._h, ctypes.c_void_p(rows_ptr or None), ctypes.c_void_p(vectors_ptr or None),
                                          int(n), MEM_DEVICE, ctypes.c_void_p(stream or None)))
        return int(n)

    def get_vectors(self, start: int = 0, n: Optional[int] = None) -> np.ndarray:
        total = self.count()
        n = total - start if n is None else n
        out = np.empty((max(n, 0), self.dim), dtype=np.float32)
        if n > 0:
            _check(self._lib.vdb_index_get_vectors(self._h, int(start), int(n), _ptr(out)))
        return out

    # -- search ----------------------------------------------------------------
    def search(self, queries: np.ndarray, k: int, row_mask: Optional[np.ndarray] = None,
               with_keys: bool = False, index_offset: int = 0):
        """Host-memory search.  Returns (scores f32 [B,k], indices i64 [B,k][, keys f64 [B,k]])."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must have shape (B, {self.dim}), got {np.shape(queries)}")
        B = q.shape[0]
        k = int(k)
        scores = np.empty((B, k), dtype=np.float32)
        idx = np.empty((B, k), dtype=np.int64)
        keys = np.empty((B, k), dtype=np.float64) if with_keys else None
        mask_p = None
        if row_mask is not None:
            m = np.ascontiguousarray(row_mask, dtype=np.uint32)
            need = (self.count() + 31) // 32
            if m.size < need:
                raise ValueError(f"row_mask needs {need} uint32 words, got {m.size}")
            mask_p = _ptr(m)
        _check(self._lib.vdb_index_search(self._h, _ptr(q), B, k, mask_p, MEM_HOST, _ptr(scores), _ptr(idx),
                                          _ptr(keys) if keys is not None else None, int(index_offset), None))
        return (scores, idx, keys) if with_keys else (scores, idx)

    def search_device(self, q_ptr: int, n_queries: int, k: int, out_scores_ptr: int, out_idx_ptr: int,
                      out_keys_ptr: int = 0, mask_ptr: int = 0, index_offset: int = 0, stream: int = 0) -> None:
        """Device-memory search (pointers from torch tensors); stream-ordered."""
        _check(self._lib.vdb_index_search(
            self._h, ctypes.c_void_p(q_ptr), int(n_queries), int(k), ctypes.c_void_p(mask_ptr or None),
            MEM_DEVICE, ctypes.c_void_p(out_scores_ptr), ctypes.c_void_p(out_idx_ptr),
            ctypes.c_void_p(out_keys_ptr or None), int(index_offset), ctypes.c_void_p(stream or None)))

    def search_rows(self, queries: np.ndarray, k: int, lists, query_list=None, with_keys: bool = False,
                    index_offset: int = 0):
        """include/vdb.h vdb_index_search_rows, host memory: query b is searched over the rows of
        ``lists[query_list[b]]`` (``lists[b]`` without a ``query_list``) only, exactly.  ``lists``: a
        sequence of integer arrays, each strictly ascending row ids in [0, count), packed to CSR
        here.  Returns what ``search`` with a ``row_mask`` of exactly that list's rows returns.  A
        malformed list or ``query_list`` raises ValueError."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must have shape (B, {self.dim}), got {np.shape(queries)}")
        offs, rows = pack_row_lists(lists)
        ql = None
        if query_list is not None:
            ql = np.asarray(query_list)
            if ql.size and ql.dtype.kind not in "iu":
                raise ValueError(f"query_list must hold integers, got dtype {ql.dtype}")
            if ql.reshape(-1).size != q.shape[0]:
                raise ValueError(f"query_list needs {q.shape[0]} entries, got {ql.size}")
            if ql.size and (int(ql.min()) < -2**31 or int(ql.max()) >= 2**31):
                raise ValueError("query_list entries must fit int32")
            ql = np.ascontiguousarray(ql.reshape(-1), dtype=np.int32)
        return self.search_rows_csr(q, k, offs, rows, ql, with_keys=with_keys, index_offset=index_offset)

    def search_rows_csr(self, q: np.ndarray, k: int, offsets: np.ndarray, rows: np.ndarray,
                        query_list: Optional[np.ndarray] = None, with_keys: bool = False, index_offset: int = 0):
        """``search_rows`` with the lists already in CSR form (int64 offsets [n_lists + 1] and rows,
        int32 query_list or None), passed to the C-ABI as they are."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        offs = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        ql = None if query_list is None else np.ascontiguousarray(query_list, dtype=np.int32).reshape(-1)
        if offs.size < 1:
            raise ValueError("offsets needs n_lists + 1 entries")
        B, k = q.shape[0], int(k)
        scores = np.empty((B, k), dtype=np.float32)
        idx = np.empty((B, k), dtype=np.int64)
        keys = np.empty((B, k), dtype=np.float64) if with_keys else None
        _check(self._lib.vdb_index_search_rows(
            self._h, _ptr(q), B, k, _ptr(offs), offs.size - 1, _ptr(rows) if rows.size else None, rows.size,
            _ptr(ql) if ql is not None else None, MEM_HOST, _ptr(scores), _ptr(idx),
            _ptr(keys) if keys is not None else None, int(index_offset), None))
        return (scores, idx, keys) if with_keys else (scores, idx)

    def search_rows_device(self, q_ptr: int, n_queries: int, k: int, offsets_ptr: int, n_lists: int, rows_ptr: int,
                           n_ids: int, out_scores_ptr: int, out_idx_ptr: int, out_keys_ptr: int = 0,
                           query_list_ptr: int = 0, index_offset: int = 0, stream: int = 0) -> None:
        """vdb_index_search_rows with device-memory arguments (int64 offsets and rows, int32
        query_list); stream-ordered, nothing is validated on the host (include/vdb.h)."""
        _check(self._lib.vdb_index_search_rows(
            self._h, ctypes.c_void_p(q_ptr), int(n_queries), int(k), ctypes.c_void_p(offsets_ptr), int(n_lists),
            ctypes.c_void_p(rows_ptr or None), int(n_ids), ctypes.c_void_p(query_list_ptr or None), MEM_DEVICE,
            ctypes.c_void_p(out_scores_ptr), ctypes.c_void_p(out_idx_ptr), ctypes.c_void_p(out_keys_ptr or None),
            int(index_offset), ctypes.c_void_p(stream or None)))

    # largest capacity a ``search_range`` call without a ``cap`` starts with
    RANGE_FIRST_CAP = 1024

    def search_range(self, queries: np.ndarray, thresholds, cap: Optional[int] = None,
                     row_mask: Optional[np.ndarray] = None, with_keys: bool = False, index_offset: int = 0):
        """include/vdb.h vdb_index_search_range, host memory: every row whose exact key is at or
        above the query's threshold (cosine: similarity >= t; euclidean: distance <= t), in
        ascending row id.  ``thresholds``: one fp64 per query, or a scalar for all of them.
        Returns (counts i64 [B], indices i64 [B, cap], scores f32 [B, cap][, keys f64 [B, cap]]):
        counts are exact even above ``cap``; slots past min(count, cap) are -1 / 0 / -inf.
        ``cap=0`` counts only.  ``cap=None``: every hit is returned -- a call with cap 1024 and,
        if a count exceeds it, one more with cap = the largest count."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must have shape (B, {self.dim}), got {np.shape(queries)}")
        B = q.shape[0]
        thr = np.asarray(thresholds, dtype=np.float64)
        if thr.ndim == 0:
            thr = np.full(B, float(thr), dtype=np.float64)
        thr = np.ascontiguousarray(thr.reshape(-1))
        if thr.size != B:
            raise ValueError(f"thresholds needs {B} entries, got {thr.size}")
        mask_p = None
        if row_mask is not None:
            m = np.ascontiguousarray(row_mask, dtype=np.uint32)
            need = (self.count() + 31) // 32
            if m.size < need:
                raise ValueError(f"row_mask needs {need} uint32 words, got {m.size}")
            mask_p = _ptr(m)

        def call(c):
            counts = np.zeros(B, dtype=np.int64)
            idx = np.empty((B, max(c, 0)), dtype=np.int64)  # (a negative cap is the library's to refuse)
            scores = np.empty((B, max(c, 0)), dtype=np.float32)
            keys = np.empty((B, max(c, 0)), dtype=np.float64) if with_keys else None
            _check(self._lib.vdb_index_search_range(
                self._h, _ptr(q), B, _ptr(thr), mask_p, MEM_HOST, c, _ptr(counts), _ptr(idx) if c > 0 else None,
                _ptr(scores) if c > 0 else None, _ptr(keys) if keys is not None and c > 0 else None,
                int(index_offset), None))
            return (counts, idx, scores, keys) if with_keys else (counts, idx, scores)

        if cap is not None:
            return call(int(cap))
        out = call(self.RANGE_FIRST_CAP)
        most = int(out[0].max()) if B else 0
        return call(most) if most > self.RANGE_FIRST_CAP else out

    def search_range_device(self, q_ptr: int, n_queries: int, thresholds_ptr: int, cap: int, out_counts_ptr: int,
                            out_idx_ptr: int = 0, out_scores_ptr: int = 0, out_keys_ptr: int = 0, mask_ptr: int = 0,
                            index_offset: int = 0, stream: int = 0) -> None:
        """vdb_index_search_range with device-memory arguments (fp32 queries, fp64 thresholds,
        int64 counts and indices); stream-ordered, nothing is read back and the thresholds are not
        validated on the host (include/vdb.h)."""
        _check(self._lib.vdb_index_search_range(
            self._h, ctypes.c_void_p(q_ptr), int(n_queries), ctypes.c_void_p(thresholds_ptr),
            ctypes.c_void_p(mask_ptr or None), MEM_DEVICE, int(cap), ctypes.c_void_p(out_counts_ptr),
            ctypes.c_void_p(out_idx_ptr or None), ctypes.c_void_p(out_scores_ptr or None),
            ctypes.c_void_p(out_keys_ptr or None), int(index_offset), ctypes.c_void_p(stream or None)))

    # -- numeric columns and predicate masks ---------------------------------------
    def set_column(self, slot: int, values) -> None:
        """include/vdb.h vdb_index_set_column, host memory: attach one fp64 value per row to
        ``slot`` (0..15; ``len(values) == count``; NaN = the row has no value).  ``None`` detaches
        the slot.  Every add, remove and clear drops all slots; an update keeps them."""
        if values is None:
            _check(self._lib.vdb_index_set_column(self._h, int(slot), None, 0, MEM_HOST, None))
            return
        v = np.ascontiguousarray(np.asarray(values, dtype=np.float64).reshape(-1))
        # (an empty array still attaches -- to an empty index: a pointer the library never reads)
        _check(self._lib.vdb_index_set_column(self._h, int(slot), _ptr(v) if v.size else _ptr(np.zeros(1, np.float64)),
                                              v.size, MEM_HOST, None))

    def set_column_device(self, slot: int, ptr: int, n: int, stream: int = 0) -> None:
        """vdb_index_set_column with a device-memory fp64 column, read after the work queued on
        ``stream``."""
        _check(self._lib.vdb_index_set_column(self._h, int(slot), ctypes.c_void_p(ptr or None), int(n), MEM_DEVICE,
                                              ctypes.c_void_p(stream or None)))

    def filter_mask(self, predicates, base_masks: Optional[np.ndarray] = None):
        """include/vdb.h vdb_index_filter_mask, host memory: ``predicates`` is a list of lists of
        ``(slot, lo, hi, flags)`` clauses, each inner list ANDed (an empty one passes every row).
        ``base_masks``: None or uint32 [P, W] ANDed into the result.  Returns (masks uint32 [P, W]
        in the row_mask layout, W = ceil(count / 32); counts int64 [P], the bits set)."""
        clauses, offsets = pack_predicates(predicates)
        P = offsets.size - 1
        W = (self.count() + 31) // 32
        base_p = None
        if base_masks is not None:
            base = np.ascontiguousarray(base_masks, dtype=np.uint32)
            if base.size != P * W:
                raise ValueError(f"base_masks needs {P} x {W} uint32 words, got {base.size}")
            base_p = _ptr(base) if base.size else None
        masks = np.zeros((P, W), dtype=np.uint32)
        counts = np.zeros(P, dtype=np.int64)
        _check(self._lib.vdb_index_filter_mask(
            self._h, _ptr(clauses) if clauses.size else None, _ptr(offsets), P, base_p, MEM_HOST,
            _ptr(masks) if masks.size else None, _ptr(counts) if P else None, None))
        return masks, counts

    def filter_mask_device(self, clauses: np.ndarray, pred_offsets: np.ndarray, base_ptr: int, out_masks_ptr: int,
                           out_counts_ptr: int = 0, stream: int = 0) -> None:
        """vdb_index_filter_mask with device-memory masks and counts (uint32 [P, W] and int64 [P]);
        ``clauses`` (FILTER_CLAUSE_DTYPE) and ``pred_offsets`` (int32 [P + 1]) are host arrays, as
        the call always takes them.  Stream-ordered, nothing is read back: an output mask can be
        the ``mask_ptr`` of a ``search_device`` queued behind it on the same stream."""
        cl = np.ascontiguousarray(clauses, dtype=FILTER_CLAUSE_DTYPE).reshape(-1)
        offs = np.ascontiguousarray(pred_offsets, dtype=np.int32).reshape(-1)
        if offs.size < 1:
            raise ValueError("pred_offsets needs n_preds + 1 entries")
        _check(self._lib.vdb_index_filter_mask(
            self._h, _ptr(cl) if cl.size else None, _ptr(offs), offs.size - 1, ctypes.c_void_p(base_ptr or None),
            MEM_DEVICE, ctypes.c_void_p(out_masks_ptr or None), ctypes.c_void_p(out_counts_ptr or None),
            ctypes.c_void_p(stream or None)))

    # -- grouped search ----------------------------------------------------------
    def set_groups(self, groups) -> None:
        """include/vdb.h vdb_index_set_groups, host memory: attach one int32 group id per row
        (``len(groups) == count``; a negative id = the row has no group).  ``None`` detaches the
        column.  Every add, remove and clear drops it; an update keeps it."""
        if groups is None:
            _check(self._lib.vdb_index_set_groups(self._h, None, 0, MEM_HOST, None))
            return
        g = np.asarray(groups)
        if g.size and g.dtype.kind not in "iu":
            raise ValueError(f"group ids must be integers, got dtype {g.dtype}")
        if g.size and (int(g.min()) < -2**31 or int(g.max()) >= 2**31):
            raise ValueError("group ids must fit int32")
        g = np.ascontiguousarray(g.reshape(-1), dtype=np.int32)
        # (an empty array still attaches -- to an empty index: a pointer the library never reads)
        _check(self._lib.vdb_index_set_groups(self._h, _ptr(g) if g.size else _ptr(np.zeros(1, np.int32)), g.size,
                                              MEM_HOST, None))

    def set_groups_device(self, ptr: int, n: int, stream: int = 0) -> None:
        """vdb_index_set_groups with a device-memory int32 column, read after the work queued on
        ``stream``."""
        _check(self._lib.vdb_index_set_groups(self._h, ctypes.c_void_p(ptr or None), int(n), MEM_DEVICE,
                                              ctypes.c_void_p(stream or None)))

    def search_groups(self, queries: np.ndarray, k: int, row_mask: Optional[np.ndarray] = None,
                      with_keys: bool = False, index_offset: int = 0):
        """include/vdb.h vdb_index_search_groups, host memory: the k best distinct groups of each
        query, slot j holding the best row of the j-th group.  Returns (scores f32 [B,k], indices
        i64 [B,k], groups i32 [B,k][, keys f64 [B,k]]); slots past the number of eligible groups
        are 0 / -1 / -1 / -inf."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must have shape (B, {self.dim}), got {np.shape(queries)}")
        B = q.shape[0]
        k = int(k)
        scores = np.empty((B, max(k, 0)), dtype=np.float32)  # (a bad k is the library's to refuse)
        idx = np.empty((B, max(k, 0)), dtype=np.int64)
        grp = np.empty((B, max(k, 0)), dtype=np.int32)
        keys = np.empty((B, max(k, 0)), dtype=np.float64) if with_keys else None
        mask_p = None
        if row_mask is not None:
            m = np.ascontiguousarray(row_mask, dtype=np.uint32)
            need = (self.count() + 31) // 32
            if m.size < need:
                raise ValueError(f"row_mask needs {need} uint32 words, got {m.size}")
            mask_p = _ptr(m)
        _check(self._lib.vdb_index_search_groups(self._h, _ptr(q), B, k, mask_p, MEM_HOST, _ptr(scores), _ptr(idx),
                                                 _ptr(grp), _ptr(keys) if keys is not None else None,
                                                 int(index_offset), None))
        return (scores, idx, grp, keys) if with_keys else (scores, idx, grp)

    def search_groups_device(self, q_ptr: int, n_queries: int, k: int, out_scores_ptr: int, out_idx_ptr: int,
                             out_groups_ptr: int, out_keys_ptr: int = 0, mask_ptr: int = 0, index_offset: int = 0,
                             stream: int = 0) -> None:
        """vdb_index_search_groups with device-memory arguments; stream-ordered, nothing is read
        back."""
        _check(self._lib.vdb_index_search_groups(
            self._h, ctypes.c_void_p(q_ptr), int(n_queries), int(k), ctypes.c_void_p(mask_ptr or None), MEM_DEVICE,
            ctypes.c_void_p(out_scores_ptr), ctypes.c_void_p(out_idx_ptr), ctypes.c_void_p(out_groups_ptr or None),
            ctypes.c_void_p(out_keys_ptr or None), int(index_offset), ctypes.c_void_p(stream or None)))

    # -- MMR search --------------------------------------------------------------
    def search_mmr(self, queries: np.ndarray, k: int, fetch_k: int, lam: float, row_mask: Optional[np.ndarray] = None,
                   with_keys: bool = False, with_mmr: bool = False, index_offset: int = 0):
        """include/vdb.h vdb_index_search_mmr, host memory: of each query's best ``fetch_k`` rows the
        ``k`` picked greedily by ``lam * relevance - (1 - lam) * (greatest similarity to a picked
        row)``, in pick order.  Returns (scores f32 [B,k], indices i64 [B,k][, keys f64 [B,k]][, mmr
        f64 [B,k]]); slots past min(k, candidates) are 0 / -1 / -inf / -inf."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must have shape (B, {self.dim}), got {np.shape(queries)}")
        B = q.shape[0]
        k = int(k)
        scores = np.empty((B, max(k, 0)), dtype=np.float32)  # (a bad k is the library's to refuse)
        idx = np.empty((B, max(k, 0)), dtype=np.int64)
        keys = np.empty((B, max(k, 0)), dtype=np.float64) if with_keys else None
        mmr = np.empty((B, max(k, 0)), dtype=np.float64) if with_mmr else None
        mask_p = None
        if row_mask is not None:
            m = np.ascontiguousarray(row_mask, dtype=np.uint32)
            need = (self.count() + 31) // 32
            if m.size < need:
                raise ValueError(f"row_mask needs {need} uint32 words, got {m.size}")
            mask_p = _ptr(m)
        _check(self._lib.vdb_index_search_mmr(self._h, _ptr(q), B, k, int(fetch_k), float(lam), mask_p, MEM_HOST,
                                              _ptr(scores), _ptr(idx), _ptr(keys) if keys is not None else None,
                                              _ptr(mmr) if mmr is not None else None, int(index_offset), None))
        out = (scores, idx)
        if with_keys:
            out += (keys,)
        if with_mmr:
            out += (mmr,)
        return out

    def search_mmr_device(self, q_ptr: int, n_queries: int, k: int, fetch_k: int, lam: float, out_scores_ptr: int,
                          out_idx_ptr: int, out_keys_ptr: int = 0, out_mmr_ptr: int = 0, mask_ptr: int = 0,
                          index_offset: int = 0, stream: int = 0) -> None:
        """vdb_index_search_mmr with device-memory arguments; stream-ordered, nothing is read back."""
        _check(self._lib.vdb_index_search_mmr(
            self._h, ctypes.c_void_p(q_ptr), int(n_queries), int(k), int(fetch_k), float(lam),
            ctypes.c_void_p(mask_ptr or None), MEM_DEVICE, ctypes.c_void_p(out_scores_ptr), ctypes.c_void_p(out_idx_ptr),
            ctypes.c_void_p(out_keys_ptr or None), ctypes.c_void_p(out_mmr_ptr or None), int(index_offset),
            ctypes.c_void_p(stream or None)))

    # -- recommend search ----------------------------------------------------------
    def search_recommend(self, positive, negative=None, k: int = 10, row_mask: Optional[np.ndarray] = None,
                         with_keys: bool = False, with_queries: bool = False, index_offset: int = 0):
        """include/vdb.h vdb_index_search_recommend, host memory: query b is built on the device
        from the stored rows ``positive[b]`` (and ``negative[b]``: their means, ``2 mp - mn``) and
        answered as ``search`` would answer that vector, the examples left out.  ``positive`` /
        ``negative``: a sequence of integer row-id sequences, one per query (``negative=None``: no
        query has negatives), packed to CSR here.  Returns (scores f32 [B,k], indices i64 [B,k][,
        keys f64 [B,k]][, queries f32 [B,dim]]); a query without a positive is all 0 / -1 / -inf.  A
        malformed list, more than 64 examples or ``k`` outside [1, 136] raises ValueError."""
        po, pr = pack_row_lists(positive)
        B = po.size - 1
        no = nr = None
        if negative is not None:
            no, nr = pack_row_lists(negative)
            if no.size - 1 != B:
                raise ValueError(f"negative needs one list per query ({B}), got {no.size - 1}")
        k = int(k)
        scores = np.empty((B, max(k, 0)), dtype=np.float32)  # (a bad k is the library's to refuse)
        idx = np.empty((B, max(k, 0)), dtype=np.int64)
        keys = np.empty((B, max(k, 0)), dtype=np.float64) if with_keys else None
        qs = np.empty((B, self.dim), dtype=np.float32) if with_queries else None
        mask_p = None
        if row_mask is not None:
            m = np.ascontiguousarray(row_mask, dtype=np.uint32)
            need = (self.count() + 31) // 32
            if m.size < need:
                raise ValueError(f"row_mask needs {need} uint32 words, got {m.size}")
            mask_p = _ptr(m)
        _check(self._lib.vdb_index_search_recommend(
            self._h, B, k, _ptr(po), _ptr(pr) if pr.size else None, pr.size,
            _ptr(no) if no is not None else None, _ptr(nr) if nr is not None and nr.size else None,
            nr.size if nr is not None else 0, mask_p, MEM_HOST, _ptr(scores), _ptr(idx),
            _ptr(keys) if keys is not None else None, _ptr(qs) if qs is not None else None, int(index_offset), None))
        out = (scores, idx)
        if with_keys:
            out += (keys,)
        if with_queries:
            out += (qs,)
        return out

    def search_recommend_device(self, n_queries: int, k: int, pos_offsets_ptr: int, pos_rows_ptr: int, n_pos: int,
                                out_scores_ptr: int, out_idx_ptr: int, neg_offsets_ptr: int = 0, neg_rows_ptr: int = 0,
                                n_neg: int = 0, out_keys_ptr: int = 0, out_queries_ptr: int = 0, mask_ptr: int = 0,
                                index_offset: int = 0, stream: int = 0) -> None:
        """vdb_index_search_recommend with device-memory arguments (int64 offsets and rows);
        stream-ordered, nothing is validated on the host and nothing is read back (a query with a bad
        list comes back empty and counts in stat ``recommend_bad_queries``)."""
        _check(self._lib.vdb_index_search_recommend(
            self._h, int(n_queries), int(k), ctypes.c_void_p(pos_offsets_ptr or None),
            ctypes.c_void_p(pos_rows_ptr or None), int(n_pos), ctypes.c_void_p(neg_offsets_ptr or None),
            ctypes.c_void_p(neg_rows_ptr or None), int(n_neg), ctypes.c_void_p(mask_ptr or None), MEM_DEVICE,
            ctypes.c_void_p(out_scores_ptr or None), ctypes.c_void_p(out_idx_ptr or None),
            ctypes.c_void_p(out_keys_ptr or None), ctypes.c_void_p(out_queries_ptr or None), int(index_offset),
            ctypes.c_void_p(stream or None)))

    # -- fused search --------------------------------------------------------------
    def search_fused(self, queries: np.ndarray, set_offsets, k: int, fetch_k: int, fusion: str = "rrf", weights=None,
                     rrf_c: float = 60.0, row_mask: Optional[np.ndarray] = None, with_fused: bool = False,
                     with_hits: bool = False, index_offset: int = 0):
        """include/vdb.h vdb_index_search_fused, host memory: set s is the sub-queries
        ``queries[set_offsets[s]:set_offsets[s + 1]]`` (``pack_query_sets`` builds the pair); each
        sub-query's best ``fetch_k`` rows are fused per row, ``fusion="rrf"``: the sum over the lists
        holding it of ``weights[l] / (rrf_c + rank)``, ``"max"``: its greatest key, and ranked by
        (fused desc, row asc).  Returns (scores f32 [S,k], indices i64 [S,k][, fused f64 [S,k]][, hits
        i32 [S,k]]); slots past min(k, candidates) are 0 / -1 / -inf / 0.  A set of more than 16
        sub-queries, a bad weight or ``k`` / ``fetch_k`` outside 1 <= k <= fetch_k <= 200 raises
        ValueError."""
        if fusion not in FUSION_IDS:
            raise ValueError(f"fusion must be one of {sorted(FUSION_IDS)}, got {fusion!r}")
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q.reshape(-1, self.dim) if q.size == 0 else q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must have shape (n_sub, {self.dim}), got {np.shape(queries)}")
        offs = np.ascontiguousarray(set_offsets, dtype=np.int64).reshape(-1)
        if offs.size < 1:
            raise ValueError("set_offsets needs n_sets + 1 entries")
        n_sub, S = q.shape[0], offs.size - 1
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
            if w.size != n_sub:
                raise ValueError(f"weights needs one entry per sub-query ({n_sub}), got {w.size}")
        k = int(k)
        scores = np.empty((S, max(k, 0)), dtype=np.float32)  # (a bad k is the library's to refuse)
        idx = np.empty((S, max(k, 0)), dtype=np.int64)
        fused = np.empty((S, max(k, 0)), dtype=np.float64) if with_fused else None
        hits = np.empty((S, max(k, 0)), dtype=np.int32) if with_hits else None
        mask_p = None
        if row_mask is not None:
            m = np.ascontiguousarray(row_mask, dtype=np.uint32)
            need = (self.count() + 31) // 32
            if m.size < need:
                raise ValueError(f"row_mask needs {need} uint32 words, got {m.size}")
            mask_p = _ptr(m)
        _check(self._lib.vdb_index_search_fused(
            self._h, _ptr(q) if n_sub else None, n_sub, _ptr(offs), S, _ptr(w) if w is not None and n_sub else None, k,
            int(fetch_k), FUSION_IDS[fusion], float(rrf_c), mask_p, MEM_HOST, _ptr(scores), _ptr(idx),
            _ptr(fused) if fused is not None else None, _ptr(hits) if hits is not None else None, int(index_offset), None))
        out = (scores, idx)
        if with_fused:
            out += (fused,)
        if with_hits:
            out += (hits,)
        return out

    def search_fused_device(self, q_ptr: int, n_sub: int, set_offsets_ptr: int, n_sets: int, k: int, fetch_k: int,
                            out_scores_ptr: int, out_idx_ptr: int, fusion: str = "rrf", weights_ptr: int = 0,
                            rrf_c: float = 60.0, out_fused_ptr: int = 0, out_hits_ptr: int = 0, mask_ptr: int = 0,
                            index_offset: int = 0, stream: int = 0) -> None:
        """vdb_index_search_fused with device-memory arguments (fp32 queries, int64 offsets, fp64
        weights); stream-ordered, the offsets and weights are not validated on the host and nothing is
        read back (a bad set comes back empty and counts in stat ``fused_bad_sets``)."""
        _check(self._lib.vdb_index_search_fused(
            self._h, ctypes.c_void_p(q_ptr or None), int(n_sub), ctypes.c_void_p(set_offsets_ptr or None), int(n_sets),
            ctypes.c_void_p(weights_ptr or None), int(k), int(fetch_k), FUSION_IDS[fusion], float(rrf_c),
            ctypes.c_void_p(mask_ptr or None), MEM_DEVICE, ctypes.c_void_p(out_scores_ptr or None),
            ctypes.c_void_p(out_idx_ptr or None), ctypes.c_void_p(out_fused_ptr or None),
            ctypes.c_void_p(out_hits_ptr or None), int(index_offset), ctypes.c_void_p(stream or None)))

    # -- sparse and hybrid search ----------------------------------------------------
    @staticmethod
    def _csr(indptr, terms, weights, what: str):
        ip = np.ascontiguousarray(indptr, dtype=np.int64).reshape(-1)
        if ip.size < 1:
            raise ValueError(f"{what} indptr needs n + 1 entries")
        t = np.asarray(terms)
        if t.size and t.dtype.kind not in "iu":
            raise ValueError(f"{what} term ids must be integers, got dtype {t.dtype}")
        if t.size and (int(t.min()) < -2**31 or int(t.max()) >= 2**31):
            raise ValueError(f"{what} term ids must fit int32")
        t = np.ascontiguousarray(t.reshape(-1), dtype=np.int32)
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        if t.size != w.size:
            raise ValueError(f"{what} terms and weights differ in length: {t.size} and {w.size}")
        return ip, t, w

    def set_sparse(self, indptr, terms=None, weights=None, n_terms: int = 0) -> None:
        """include/vdb.h vdb_index_set_sparse, host memory: attach one sparse vector per row in CSR
        form (``len(indptr) == count + 1``; row r's entries are ``terms / weights[indptr[r]:
        indptr[r + 1]]``, term ids strictly ascending in [0, ``n_terms``), weights finite).
        ``indptr=None`` detaches the column.  Every add, remove and clear drops it; an update keeps
        it.  A column the library refuses raises ValueError and leaves the earlier one attached."""
        if indptr is None:
            _check(self._lib.vdb_index_set_sparse(self._h, None, None, None, 0, 0, 0, MEM_HOST, None))
            return
        ip, t, w = self._csr(indptr, terms if terms is not None else (), weights if weights is not None else (), "sparse column")
        _check(self._lib.vdb_index_set_sparse(self._h, _ptr(ip), _ptr(t) if t.size else None, _ptr(w) if w.size else None,
                                              ip.size - 1, t.size, int(n_terms), MEM_HOST, None))

    def set_sparse_device(self, indptr_ptr: int, terms_ptr: int, weights_ptr: int, n: int, nnz: int, n_terms: int,
                          stream: int = 0) -> None:
        """vdb_index_set_sparse with a device-memory column (int64 indptr, int32 terms, fp32 weights),
        read after the work queued on ``stream`` and validated by a kernel."""
        _check(self._lib.vdb_index_set_sparse(self._h, ctypes.c_void_p(indptr_ptr or None), ctypes.c_void_p(terms_ptr or None),
                                              ctypes.c_void_p(weights_ptr or None), int(n), int(nnz), int(n_terms),
                                              MEM_DEVICE, ctypes.c_void_p(stream or None)))

    def _mask_ptr(self, row_mask):
        if row_mask is None:
            return None, None
        m = np.ascontiguousarray(row_mask, dtype=np.uint32)
        need = (self.count() + 31) // 32
        if m.size < need:
            raise ValueError(f"row_mask needs {need} uint32 words, got {m.size}")
        return m, _ptr(m)

    def search_sparse(self, q_indptr, q_terms, q_weights, k: int, row_mask: Optional[np.ndarray] = None,
                      with_keys: bool = False, index_offset: int = 0):
        """include/vdb.h vdb_index_search_sparse, host memory: query b is the sparse vector
        ``q_terms / q_weights[q_indptr[b]:q_indptr[b + 1]]`` (``pack_sparse_vectors`` builds the
        triple; at most 1 024 terms, ids strictly ascending); the rows that share a term with it rank
        by (fp64 dot product desc, row asc).  Returns (scores f32 [B,k], indices i64 [B,k][, keys f64
        [B,k]]); slots past min(k, matching rows) are 0 / -1 / -inf.  Needs a column (``set_sparse``);
        ``k`` outside [1, 1024] or a bad query raises ValueError."""
        ip, t, w = self._csr(q_indptr, q_terms, q_weights, "query")
        B, k = ip.size - 1, int(k)
        scores = np.empty((B, max(k, 0)), dtype=np.float32)  # (a bad k is the library's to refuse)
        idx = np.empty((B, max(k, 0)), dtype=np.int64)
        keys = np.empty((B, max(k, 0)), dtype=np.float64) if with_keys else None
        m, mask_p = self._mask_ptr(row_mask)
        _check(self._lib.vdb_index_search_sparse(
            self._h, _ptr(ip), _ptr(t) if t.size else None, _ptr(w) if w.size else None, B, t.size, k, mask_p, MEM_HOST,
            _ptr(scores), _ptr(idx), _ptr(keys) if keys is not None else None, int(index_offset), None))
        return (scores, idx, keys) if with_keys else (scores, idx)

    def search_sparse_device(self, q_indptr_ptr: int, q_terms_ptr: int, q_weights_ptr: int, n_queries: int, q_nnz: int,
                             k: int, out_scores_ptr: int, out_idx_ptr: int, out_keys_ptr: int = 0, mask_ptr: int = 0,
                             index_offset: int = 0, stream: int = 0) -> None:
        """vdb_index_search_sparse with device-memory arguments; stream-ordered, the queries are not
        validated on the host and nothing is read back (a bad query comes back empty and counts in stat
        ``sparse_bad_queries``)."""
        _check(self._lib.vdb_index_search_sparse(
            self._h, ctypes.c_void_p(q_indptr_ptr or None), ctypes.c_void_p(q_terms_ptr or None),
            ctypes.c_void_p(q_weights_ptr or None), int(n_queries), int(q_nnz), int(k), ctypes.c_void_p(mask_ptr or None),
            MEM_DEVICE, ctypes.c_void_p(out_scores_ptr or None), ctypes.c_void_p(out_idx_ptr or None),
            ctypes.c_void_p(out_keys_ptr or None), int(index_offset), ctypes.c_void_p(stream or None)))

    def search_hybrid(self, queries: np.ndarray, q_indptr, q_terms, q_weights, k: int, fetch_k: int,
                      weights=(1.0, 1.0), rrf_c: float = 60.0, row_mask: Optional[np.ndarray] = None,
                      with_fused: bool = False, with_hits: bool = False, index_offset: int = 0):
        """include/vdb.h vdb_index_search_hybrid, host memory: query b fuses the best ``fetch_k`` rows
        of the dense search for ``queries[b]`` with the best ``fetch_k`` of the sparse search for
        sparse query b by weighted reciprocal rank, ``weights = (w_dense, w_sparse)``, and ranks by
        (fused desc, row asc).  Returns (scores f32 [B,k], indices i64 [B,k][, fused f64 [B,k]][, hits
        i32 [B,k]]).  ``k`` / ``fetch_k`` outside 1 <= k <= fetch_k <= 200, a bad weight or a bad query
        raises ValueError."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q.reshape(-1, self.dim) if q.size == 0 else q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must have shape (n_queries, {self.dim}), got {np.shape(queries)}")
        ip, t, w = self._csr(q_indptr, q_terms, q_weights, "query")
        B, k = ip.size - 1, int(k)
        if q.shape[0] != B:
            raise ValueError(f"{q.shape[0]} dense queries but {B} sparse ones")
        if len(weights) != 2:
            raise ValueError("weights must be (w_dense, w_sparse)")
        scores = np.empty((B, max(k, 0)), dtype=np.float32)
        idx = np.empty((B, max(k, 0)), dtype=np.int64)
        fused = np.empty((B, max(k, 0)), dtype=np.float64) if with_fused else None
        hits = np.empty((B, max(k, 0)), dtype=np.int32) if with_hits else None
        m, mask_p = self._mask_ptr(row_mask)
        _check(self._lib.vdb_index_search_hybrid(
            self._h, _ptr(q) if B else None, _ptr(ip), _ptr(t) if t.size else None, _ptr(w) if w.size else None, B, t.size,
            k, int(fetch_k), float(weights[0]), float(weights[1]), float(rrf_c), mask_p, MEM_HOST, _ptr(scores), _ptr(idx),
            _ptr(fused) if fused is not None else None, _ptr(hits) if hits is not None else None, int(index_offset), None))
        out = (scores, idx)
        if with_fused:
            out += (fused,)
        if with_hits:
            out += (hits,)
        return out

    def search_hybrid_device(self, q_ptr: int, q_indptr_ptr: int, q_terms_ptr: int, q_weights_ptr: int, n_queries: int,
                             q_nnz: int, k: int, fetch_k: int, out_scores_ptr: int, out_idx_ptr: int,
                             weights=(1.0, 1.0), rrf_c: float = 60.0, out_fused_ptr: int = 0, out_hits_ptr: int = 0,
                             mask_ptr: int = 0, index_offset: int = 0, stream: int = 0) -> None:
        """vdb_index_search_hybrid with device-memory arguments; stream-ordered, nothing is read back
        (a bad sparse query contributes an empty sparse list and counts in ``sparse_bad_queries``)."""
        _check(self._lib.vdb_index_search_hybrid(
            self._h, ctypes.c_void_p(q_ptr or None), ctypes.c_void_p(q_indptr_ptr or None),
            ctypes.c_void_p(q_terms_ptr or None), ctypes.c_void_p(q_weights_ptr or None), int(n_queries), int(q_nnz),
            int(k), int(fetch_k), float(weights[0]), float(weights[1]), float(rrf_c), ctypes.c_void_p(mask_ptr or None),
            MEM_DEVICE, ctypes.c_void_p(out_scores_ptr or None), ctypes.c_void_p(out_idx_ptr or None),
            ctypes.c_void_p(out_fused_ptr or None), ctypes.c_void_p(out_hits_ptr or None), int(index_offset),
            ctypes.c_void_p(stream or None)))

    def search_hybrid_sum(self, queries: np.ndarray, q_indptr, q_terms, q_weights, k: int, weights=(1.0, 1.0),
                          row_mask: Optional[np.ndarray] = None, with_fused: bool = False, with_parts: bool = False,
                          index_offset: int = 0):
        """include/vdb.h vdb_index_search_hybrid_sum, host memory: every row whose mask bit is set is
        ranked by ``(w_dense * kd + w_sparse * ks) + 0.0`` in fp64, ``kd`` the dense key of
        ``queries[b]`` (cosine similarity, or minus the squared distance) and ``ks`` the sparse dot
        product with sparse query b, ``weights = (w_dense, w_sparse)`` each in [0, 2^64]; the exact top
        ``k`` of the whole corpus by (value desc, row asc).  Returns (scores f32 [B,k], indices i64
        [B,k][, fused f64 [B,k]][, dense f64 [B,k], sparse f64 [B,k]]); slots past min(k, eligible rows)
        are 0 / -1 / -inf.  ``k`` outside [1, 1024], a bad weight or a bad query raises ValueError."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q.reshape(-1, self.dim) if q.size == 0 else q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must have shape (n_queries, {self.dim}), got {np.shape(queries)}")
        ip, t, w = self._csr(q_indptr, q_terms, q_weights, "query")
        B, k = ip.size - 1, int(k)
        if q.shape[0] != B:
            raise ValueError(f"{q.shape[0]} dense queries but {B} sparse ones")
        if len(weights) != 2:
            raise ValueError("weights must be (w_dense, w_sparse)")
        shape = (B, max(k, 0))  # (a bad k is the library's to refuse)
        scores = np.empty(shape, dtype=np.float32)
        idx = np.empty(shape, dtype=np.int64)
        fused = np.empty(shape, dtype=np.float64) if with_fused else None
        dense = np.empty(shape, dtype=np.float64) if with_parts else None
        sparse = np.empty(shape, dtype=np.float64) if with_parts else None
        m, mask_p = self._mask_ptr(row_mask)
        _check(self._lib.vdb_index_search_hybrid_sum(
            self._h, _ptr(q) if B else None, _ptr(ip), _ptr(t) if t.size else None, _ptr(w) if w.size else None, B, t.size,
            k, float(weights[0]), float(weights[1]), mask_p, MEM_HOST, _ptr(scores), _ptr(idx),
            _ptr(fused) if fused is not None else None, _ptr(dense) if dense is not None else None,
            _ptr(sparse) if sparse is not None else None, int(index_offset), None))
        out = (scores, idx)
        if with_fused:
            out += (fused,)
        if with_parts:
            out += (dense, sparse)
        return out

    def search_hybrid_sum_device(self, q_ptr: int, q_indptr_ptr: int, q_terms_ptr: int, q_weights_ptr: int,
                                 n_queries: int, q_nnz: int, k: int, out_scores_ptr: int, out_idx_ptr: int,
                                 weights=(1.0, 1.0), out_fused_ptr: int = 0, out_dense_ptr: int = 0,
                                 out_sparse_ptr: int = 0, mask_ptr: int = 0, index_offset: int = 0,
                                 stream: int = 0) -> None:
        """vdb_index_search_hybrid_sum with device-memory arguments; stream-ordered, nothing is read
        back (a bad sparse query comes back empty and counts in stat ``sparse_bad_queries``)."""
        _check(self._lib.vdb_index_search_hybrid_sum(
            self._h, ctypes.c_void_p(q_ptr or None), ctypes.c_void_p(q_indptr_ptr or None),
            ctypes.c_void_p(q_terms_ptr or None), ctypes.c_void_p(q_weights_ptr or None), int(n_queries), int(q_nnz),
            int(k), float(weights[0]), float(weights[1]), ctypes.c_void_p(mask_ptr or None), MEM_DEVICE,
            ctypes.c_void_p(out_scores_ptr or None), ctypes.c_void_p(out_idx_ptr or None),
            ctypes.c_void_p(out_fused_ptr or None), ctypes.c_void_p(out_dense_ptr or None),
            ctypes.c_void_p(out_sparse_ptr or None), int(index_offset), ctypes.c_void_p(stream or None)))

    # -- MaxSim search -------------------------------------------------------------
    def _maxsim_sets(self, query_sets):
        """``query_sets``: a sequence of sets, each [m, dim] (``pack_query_sets``), or the packed
        pair as a tuple ``(Q [n_sub, dim], offsets [n_sets + 1])`` -> (Q fp32, offsets int64)."""
        if isinstance(query_sets, tuple) and len(query_sets) == 2:
            o = np.asarray(query_sets[1])
            if o.ndim == 1 and o.dtype.kind in "iu":
                q = np.ascontiguousarray(query_sets[0], dtype=np.float32)
                if q.ndim == 1:
                    q = q.reshape(-1, self.dim) if q.size == 0 else q[None, :]
                if q.ndim != 2 or q.shape[1] != self.dim:
                    raise ValueError(f"queries must have shape (n_sub, {self.dim}), got {np.shape(query_sets[0])}")
                offs = np.ascontiguousarray(o, dtype=np.int64)
                if offs.size < 1:
                    raise ValueError("set_offsets needs n_sets + 1 entries")
                return q, offs
        return pack_query_sets(query_sets, self.dim)

    def search_maxsim(self, query_sets, n_group_slots: int, k: int, row_mask: Optional[np.ndarray] = None,
                      with_sums: bool = False):
        """include/vdb.h vdb_index_search_maxsim, host memory: for each set of query vectors the ``k``
        groups (``set_groups``; their ids must lie in [0, ``n_group_slots``)) with the greatest sum,
        over the set's vectors, of the vector's best canonical key among the group's rows, by (sum
        desc, group id asc).  ``query_sets`` is a sequence of sets, each [m, dim], or the packed tuple
        ``(Q, offsets)``.  Returns (scores f32 [S,k], groups i32 [S,k][, sums f64 [S,k]]), the scores
        in key units; slots past min(k, candidates) are 0 / -1 / -inf.  A set of more than 64
        vectors, ``k`` outside [1, 128] or a bad ``n_group_slots`` raises ValueError."""
        q, offs = self._maxsim_sets(query_sets)
        n_sub, S = q.shape[0], offs.size - 1
        k = int(k)
        scores = np.empty((S, max(k, 0)), dtype=np.float32)  # (a bad k is the library's to refuse)
        grp = np.empty((S, max(k, 0)), dtype=np.int32)
        sums = np.empty((S, max(k, 0)), dtype=np.float64) if with_sums else None
        mask_p = None
        if row_mask is not None:
            m = np.ascontiguousarray(row_mask, dtype=np.uint32)
            need = (self.count() + 31) // 32
            if m.size < need:
                raise ValueError(f"row_mask needs {need} uint32 words, got {m.size}")
            mask_p = _ptr(m)
        _check(self._lib.vdb_index_search_maxsim(
            self._h, _ptr(q) if n_sub else None, n_sub, _ptr(offs), S, int(n_group_slots), k, mask_p, MEM_HOST,
            _ptr(scores), _ptr(grp), _ptr(sums) if sums is not None else None, None))
        return (scores, grp, sums) if with_sums else (scores, grp)

    def search_maxsim_device(self, q_ptr: int, n_sub: int, set_offsets_ptr: int, n_sets: int, n_group_slots: int,
                             k: int, out_scores_ptr: int, out_groups_ptr: int, out_sums_ptr: int = 0,
                             mask_ptr: int = 0, stream: int = 0) -> None:
        """vdb_index_search_maxsim with device-memory arguments (fp32 queries, int64 offsets);
        stream-ordered, the offsets are not validated on the host and nothing is read back (a bad set
        comes back empty and counts in stat ``maxsim_bad_sets``)."""
        _check(self._lib.vdb_index_search_maxsim(
            self._h, ctypes.c_void_p(q_ptr or None), int(n_sub), ctypes.c_void_p(set_offsets_ptr or None), int(n_sets),
            int(n_group_slots), int(k), ctypes.c_void_p(mask_ptr or None), MEM_DEVICE,
            ctypes.c_void_p(out_scores_ptr or None), ctypes.c_void_p(out_groups_ptr or None),
            ctypes.c_void_p(out_sums_ptr or None), ctypes.c_void_p(stream or None)))


class NativeShards:
    """One corpus row-sharded over several GPUs of this process (include/vdb.h vdb_shards_*):
    the same interface as NativeIndex for the store; results identical to one index."""

    def __init__(self, dim: int, metric: str = "cosine", devices=(0,), precision: Optional[str] = None):
        if metric not in METRIC_IDS:
            raise ValueError(f"unsupported metric {metric!r}; the vdb core implements {sorted(METRIC_IDS)}")
        devices = [int(d) for d in devices]
        if not devices:
            raise ValueError("devices must name at least one GPU")
        self._lib = load_library()
        self.dim = int(dim)
        self.metric = metric
        self.devices = devices
        dv = (ctypes.c_int32 * len(devices))(*devices)
        h = ctypes.c_void_p()
        _check(self._lib.vdb_shards_create(self.dim, METRIC_IDS[metric], dv, len(devices), ctypes.byref(h)))
        self._h = h
        if precision is not None:
            self.set_param("precision", PRECISION_IDS[precision])

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.vdb_shards_destroy(h)

    def __del__(self):  # pragma: no cover - GC timing
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, rows: int) -> None:
        _check(self._lib.vdb_shards_reserve(self._h, int(rows)))

    def set_param(self, name: str, value: int) -> None:
        _check(self._lib.vdb_shards_set_param(self._h, name.encode(), int(value)))

    def stat(self, name: str) -> int:
        v = ctypes.c_int64(0)
        _check(self._lib.vdb_shards_get_stat(self._h, name.encode(), ctypes.byref(v)))
        return int(v.value)

    def shard_counts(self):
        out = []
        for g in range(len(self.devices)):
            v = ctypes.c_int64(0)
            _check(self._lib.vdb_shards_shard_count(self._h, g, ctypes.byref(v)))
            out.append(int(v.value))
        return out

    def add(self, vectors: np.ndarray) -> None:
        v = np.ascontiguousarray(vectors, dtype=np.float32)
        if v.ndim != 2 or v.shape[1] != self.dim:
            raise ValueError(f"vectors must have shape (n, {self.dim}), got {v.shape}")
        if v.shape[0]:
            _check(self._lib.vdb_shards_add(self._h, _ptr(v), v.shape[0]))

    def count(self) -> int:
        n = ctypes.c_int64(0)
        _check(self._lib.vdb_shards_count(self._h, ctypes.byref(n)))
        return int(n.value)

    def clear(self) -> None:
        _check(self._lib.vdb_shards_clear(self._h))

    def get_vectors(self, start: int = 0, n: Optional[int] = None) -> np.ndarray:
        total = self.count()
        n = total - start if n is None else n
        out = np.empty((max(n, 0), self.dim), dtype=np.float32)
        if n > 0:
            _check(self._lib.vdb_shards_get_vectors(self._h, int(start), int(n), _ptr(out)))
        return out

    def search(self, queries: np.ndarray, k: int, row_mask: Optional[np.ndarray] = None, with_keys: bool = False):
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must have shape (B, {self.dim}), got {np.shape(queries)}")
        B, k = q.shape[0], int(k)
        scores = np.empty((B, k), dtype=np.float32)
        idx = np.empty((B, k), dtype=np.int64)
        keys = np.empty((B, k), dtype=np.float64) if with_keys else None
        mask_p = None
        if row_mask is not None:
            m = np.ascontiguousarray(row_mask, dtype=np.uint32)
            need = (self.count() + 31) // 32
            if m.size < need:
                raise ValueError(f"row_mask needs {need} uint32 words, got {m.size}")
            mask_p = _ptr(m)
        _check(self._lib.vdb_shards_search(self._h, _ptr(q), B, k, mask_p, _ptr(scores), _ptr(idx),
                                           _ptr(keys) if keys is not None else None))
        return (scores, idx, keys) if with_keys else (scores, idx)


def _shards_search_device(self, q_ptr: int, n_queries: int, k: int, out_scores_ptr: int, out_idx_ptr: int,
                          out_keys_ptr: int = 0, mask_ptr: int = 0, stream: int = 0) -> None:
    """Stream-ordered search of every shard (all pointers on devices[0], no host wait)."""
    _check(self._lib.vdb_shards_search_device(
        self._h, ctypes.c_void_p(q_ptr), int(n_queries), int(k), ctypes.c_void_p(mask_ptr or None),
        ctypes.c_void_p(out_scores_ptr), ctypes.c_void_p(out_idx_ptr), ctypes.c_void_p(out_keys_ptr or None),
        ctypes.c_void_p(stream or None)))


NativeShards.search_device = _shards_search_device


def shutdown() -> None:
    """include/vdb.h vdb_shutdown: release idle workspaces of every live index."""
    _check(load_library().vdb_shutdown())


class NativeGraph:
    """The graph index over a NativeIndex's rows (include/vdb.h vdb_graph_*):
    hnswlib-style search results (labels, distances: cosine 1 - cos, L2 squared)."""

    def __init__(self, index: "NativeIndex", handle):
        self.index = index  # keeps the corpus alive
        self._lib = index._lib
        self._h = handle

    @classmethod
    def build(cls, index: "NativeIndex", degree: int = 32, knn: int = 32, n_entries: int = 256) -> "NativeGraph":
        h = ctypes.c_void_p()
        _check(index._lib.vdb_graph_build(index._h, int(degree), int(knn), int(n_entries), ctypes.byref(h)))
        return cls(index, h)

    @classmethod
    def from_arrays(cls, index: "NativeIndex", neighbors: np.ndarray, entries: np.ndarray) -> "NativeGraph":
        nb = np.ascontiguousarray(neighbors, dtype=np.int32)
        en = np.ascontiguousarray(entries, dtype=np.int32)
        if nb.ndim != 2:
            raise ValueError(f"neighbors must be [n, degree], got {nb.shape}")
        h = ctypes.c_void_p()
        _check(index._lib.vdb_graph_import(index._h, nb.shape[1], nb.shape[0], _ptr(nb) if nb.size else None,
                                           en.size, _ptr(en) if en.size else None, ctypes.byref(h)))
        return cls(index, h)

    def add(self) -> None:
        """include/vdb.h vdb_graph_add: insert the rows the index gained since the last
        build / add (incremental, instead of a rebuild)."""
        _check(self._lib.vdb_graph_add(self._h))

    def info(self) -> Tuple[int, int, int]:
        n, d, e = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int32(0)
        _check(self._lib.vdb_graph_info(self._h, ctypes.byref(n), ctypes.byref(d), ctypes.byref(e)))
        return int(n.value), int(d.value), int(e.value)

    def to_arrays(self) -> Tuple[np.ndarray, np.ndarray]:
        n, d, e = self.info()
        nb = np.empty((n, d), np.int32)
        en = np.empty(e, np.int32)
        _check(self._lib.vdb_graph_export(self._h, _ptr(nb) if nb.size else None, _ptr(en) if en.size else None))
        return nb, en

    def search(self, queries: np.ndarray, k: int, ef: int = 100):
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.index.dim:
            raise ValueError(f"queries must have shape (n, {self.index.dim}), got {np.shape(queries)}")
        labels = np.empty((q.shape[0], int(k)), np.int64)
        dist = np.empty((q.shape[0], int(k)), np.float32)
        _check(self._lib.vdb_graph_search(self._h, _ptr(q), q.shape[0], int(k), int(ef), MEM_HOST, _ptr(labels),
                                          _ptr(dist), None))
        return labels, dist

    def search_device(self, q_ptr: int, n_queries: int, k: int, ef: int, labels_ptr: int, dist_ptr: int,
                      stream: int = 0) -> None:
        _check(self._lib.vdb_graph_search(self._h, ctypes.c_void_p(q_ptr), int(n_queries), int(k), int(ef), MEM_DEVICE,
                                          ctypes.c_void_p(labels_ptr), ctypes.c_void_p(dist_ptr),
                                          ctypes.c_void_p(stream or None)))

    def stat(self, name: str) -> int:
        v = ctypes.c_int64(0)
        _check(self._lib.vdb_graph_stat(self._h, name.encode(), ctypes.byref(v)))
        return int(v.value)

    def set_param(self, name: str, value: int) -> None:
        """include/vdb.h vdb_graph_set_param ("teams": workgroups per query)."""
        _check(self._lib.vdb_graph_set_param(self._h, name.encode(), int(value)))

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.vdb_graph_destroy(h)

    def __del__(self):  # pragma: no cover - GC timing
        try:
            self.close()
        except Exception:
            pass


def merge_topk_device(keys_ptr: int, idx_ptr: int, n_lists: int, n_queries: int, k_in: int, k_out: int,
                      metric: str, out_scores_ptr: int, out_idx_ptr: int, out_keys_ptr: int = 0,
                      stream: int = 0) -> None:
    lib = load_library()
    _check(lib.vdb_merge_topk(ctypes.c_void_p(keys_ptr), ctypes.c_void_p(idx_ptr), int(n_lists), int(n_queries),
                              int(k_in), int(k_out), METRIC_IDS[metric], ctypes.c_void_p(out_scores_ptr),
                              ctypes.c_void_p(out_idx_ptr), ctypes.c_void_p(out_keys_ptr or None),
                              ctypes.c_void_p(stream or None)))


# the operator slot also serves the dot product (performance/mlx_optimized.py:150-156)
OP_METRIC_IDS = dict(METRIC_IDS, dot_product=2)


def similarity_matrix_device(corpus_ptr: int, n: int, dim: int, q_ptr: int, n_queries: int, metric: str,
                             out_ptr: int, stream: int = 0) -> None:
    lib = load_library()
    _check(lib.vdb_similarity_matrix(ctypes.c_void_p(corpus_ptr), int(n), int(dim), ctypes.c_void_p(q_ptr),
                                     int(n_queries), OP_METRIC_IDS[metric], ctypes.c_void_p(out_ptr),
                                     ctypes.c_void_p(stream or None)))


def normalize_rows_device(in_ptr: int, n: int, dim: int, out_ptr: int, stream: int = 0) -> None:
    _check(load_library().vdb_normalize_rows(ctypes.c_void_p(in_ptr), int(n), int(dim), ctypes.c_void_p(out_ptr),
                                             ctypes.c_void_p(stream or None)))


def topk_scores_device(scores_ptr: int, rows: int, n: int, k: int, largest: bool, out_idx_ptr: int,
                       out_val_ptr: int = 0, stream: int = 0) -> None:
    _check(load_library().vdb_topk_scores(ctypes.c_void_p(scores_ptr), int(rows), int(n), int(k), int(bool(largest)),
                                          ctypes.c_void_p(out_idx_ptr), ctypes.c_void_p(out_val_ptr or None),
                                          ctypes.c_void_p(stream or None)))
