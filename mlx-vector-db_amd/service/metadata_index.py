"""Metadata filter as row bitmaps, maintained at add time.

The reference filters by scanning every metadata dict on every query
(service/optimized_vector_store.py:159-165: ``[i for i, m in enumerate(meta) if
all(m.get(k) == v for k, v in filter.items())]``), O(N) Python per query.  Here
each (key, value) pair keeps a posting list of the rows holding it, appended
when rows are added; a filter is the AND of its pairs' postings, turned into the
uint32 row bitmap the device top-k consumes (include/vdb.h ``row_mask``) and
cached per (filter, row count).  A filtered query costs O(matching rows), not
O(N) dict lookups.

Semantics are exactly ``meta.get(key) == value``:
  * dict lookup finds equal hashable values (1 == 1.0 == True hash alike, as
    ``==`` treats them);
  * ``value is None`` also matches rows that lack the key (``get`` returns None);
  * a filter value that is unhashable or NaN (where dict lookup and ``==``
    disagree) falls back to the reference's scan for that pair.

A value that is a condition (service/filter_ops.py: a non-empty dict whose keys all start with
``$``) is answered from the same postings: $eq / $ne / $in / $nin / $exists as unions and
complements of posting lists, the range operators over the key's distinct numeric values
(``range_rows``); ``numeric_column`` is the fp64 column of a key that the device evaluates range
clauses on (include/vdb.h vdb_index_set_column).
"""
from __future__ import annotations

import math
import threading
from array import array
from collections import OrderedDict
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from .filter_ops import RANGE_OPS, canonical_key, has_range_ops, is_condition, parse_condition


def _hashable(v: Any) -> bool:
    try:
        hash(v)
    except TypeError:
        return False
    return not (isinstance(v, float) and math.isnan(v))


class MetadataIndex:
    """Posting lists key -> value -> rows (int64), plus rows lacking each key."""

    CACHE = 64  # bitmaps kept (LRU), keyed by (filter, row count)

    def __init__(self):
        self._post: Dict[str, Dict[Any, array]] = {}
        self._seen_rows: Dict[str, int] = {}  # key -> rows holding it (for the None / missing case)
        self._n = 0
        self._rows: List[Dict] = []
        self.version = 0  # bumped by every extend, remove, replace and clear: what a derived column is tagged with
        self._lock = threading.Lock()
        self._cache: "OrderedDict[Tuple, Tuple[np.ndarray, int]]" = OrderedDict()

    def __len__(self) -> int:
        return self._n

    def clear(self) -> None:
        with self._lock:
            self._post.clear()
            self._seen_rows.clear()
            self._n = 0
            self._rows = []
            self._cache.clear()
            self.version += 1

    def extend(self, metadata: List[Dict]) -> None:
        """Index rows [n, n + len(metadata)) (called under the store's write lock)."""
        with self._lock:
            r = self._n
            for m in metadata:
                if isinstance(m, dict):
                    for k, v in m.items():
                        if not _hashable(v):
                            continue  # never equal to a hashable filter value; unhashable filters scan
                        by_val = self._post.get(k)
                        if by_val is None:
                            by_val = self._post[k] = {}
                        lst = by_val.get(v)
                        if lst is None:
                            lst = by_val[v] = array("q")
                        lst.append(r)
                r += 1
            self._rows.extend(metadata)
            self._n = r
            self._cache.clear()
            self.version += 1

    def remove(self, rows) -> int:
        """Drop the given rows (ids in [0, len), any order, repeats allowed): the survivors keep
        their order and row r becomes r - (removed rows below r), as the device index renumbers
        them (include/vdb.h vdb_index_remove).  The postings are renumbered in place of a
        rebuild, O(total postings); every cached bitmap is dropped.  Returns the rows removed
        (called under the store's write lock)."""
        with self._lock:
            n = self._n
            ids = np.unique(np.asarray(rows, dtype=np.int64).reshape(-1))
            if ids.size and (ids[0] < 0 or ids[-1] >= n):
                raise ValueError(f"row ids must be in [0, {n}), got [{int(ids[0])}, {int(ids[-1])}]")
            self._cache.clear()
            self.version += 1
            if ids.size == 0:
                return 0
            gone = np.zeros(n, bool)
            gone[ids] = True
            below = np.cumsum(gone) - gone  # removed rows below each row
            for key in list(self._post):
                by_val = self._post[key]
                for val in list(by_val):
                    a = np.frombuffer(by_val[val], dtype=np.int64)
                    a = a[~gone[a]]
                    if a.size:
                        lst = array("q")
                        lst.frombytes((a - below[a]).astype(np.int64).tobytes())
                        by_val[val] = lst
                    else:
                        del by_val[val]
                if not by_val:
                    del self._post[key]
            self._rows = [m for m, g in zip(self._rows, gone.tolist()) if not g]
            self._n = n - int(ids.size)
            return int(ids.size)

    def rows_with(self, key: Any, value: Any) -> np.ndarray:
        """Sorted rows whose metadata has ``key`` with a value equal to ``value`` (dict-lookup
        equality, as the postings keep it), straight from the postings: no bitmap is built.  A
        row lacking the key never matches (unlike a filter on None); an unhashable or NaN value
        is held by no posting and matches nothing."""
        with self._lock:
            if not (_hashable(key) and _hashable(value)):
                return np.zeros(0, np.int64)
            lst = self._post.get(key, {}).get(value)
            if lst is None:
                return np.zeros(0, np.int64)
            return np.sort(np.frombuffer(lst, dtype=np.int64))

    def group_column(self, key: Any, n: int) -> Tuple[np.ndarray, List[Any]]:
        """(int32 [n] group id per row, values): row r's id is the position in ``values`` of its
        metadata's value for ``key``; the ids are 0..G-1 in the order of each value's first row.  A
        row without the key, or holding it with a value the postings skip (unhashable, NaN), gets
        -1: the column the device's grouped search takes (include/vdb.h vdb_index_set_groups).
        Built from the postings of ``key`` alone, O(rows holding it), not by a scan of the dicts."""
        col = np.full(max(int(n), 0), -1, dtype=np.int32)
        with self._lock:
            by_val = self._post.get(key) if _hashable(key) else None
            if not by_val:
                return col, []
            firsts = []
            for val, lst in by_val.items():
                a = np.frombuffer(lst, dtype=np.int64)
                a = a[a < n]
                if a.size:
                    firsts.append((int(a.min()), val, a))
            firsts.sort(key=lambda t: t[0])  # (a row holds one value per key: the first rows differ)
            values = []
            for gid, (_, val, a) in enumerate(firsts):
                col[a] = gid
                values.append(val)
            return col, values

    def replace(self, rows, metadata: List[Dict]) -> None:
        """Row rows[i] now has metadata[i] (ids in [0, len), pairwise distinct): the postings lose
        the old dicts' pairs and gain the new ones', O(pairs of those rows) dictionary work plus
        one pass over each posting list touched; no row is renumbered.  Every cached bitmap is
        dropped (called under the store's write lock)."""
        with self._lock:
            ids = [int(r) for r in np.asarray(rows, dtype=np.int64).reshape(-1)]
            if len(ids) != len(metadata):
                raise ValueError(f"{len(ids)} rows but {len(metadata)} metadata entries")
            if len(set(ids)) != len(ids):
                raise ValueError("row ids must be pairwise distinct")
            if ids and (min(ids) < 0 or max(ids) >= self._n):
                raise ValueError(f"row ids must be in [0, {self._n}), got [{min(ids)}, {max(ids)}]")
            self._cache.clear()
            self.version += 1
            if len(self._rows) < self._n:  # (fewer metadata entries than rows: the rest hold nothing)
                self._rows.extend({} for _ in range(self._n - len(self._rows)))
            lose: Dict[Tuple[Any, Any], set] = {}
            gain: Dict[Tuple[Any, Any], List[int]] = {}
            for r, new in zip(ids, metadata):
                old = self._rows[r]
                op = {(k, v) for k, v in old.items() if _hashable(v)} if isinstance(old, dict) else set()
                np_ = {(k, v) for k, v in new.items() if _hashable(v)} if isinstance(new, dict) else set()
                for kv in op - np_:  # (a pair both dicts hold keeps its posting entry)
                    lose.setdefault(kv, set()).add(r)
                for kv in np_ - op:
                    gain.setdefault(kv, []).append(r)
                self._rows[r] = new
            for (k, v), gone in lose.items():
                by_val = self._post.get(k)
                lst = by_val.get(v) if by_val is not None else None
                if lst is None:
                    continue
                a = np.frombuffer(lst, dtype=np.int64)
                a = a[~np.isin(a, np.fromiter(gone, dtype=np.int64, count=len(gone)))]
                if a.size:
                    kept = array("q")
                    kept.frombytes(a.astype(np.int64).tobytes())
                    by_val[v] = kept
                else:
                    del by_val[v]
                    if not by_val:
                        del self._post[k]
            for (k, v), add in gain.items():
                by_val = self._post.setdefault(k, {})
                lst = by_val.get(v)
                a = np.frombuffer(lst, dtype=np.int64) if lst is not None else np.zeros(0, np.int64)
                a = np.union1d(a, np.asarray(add, dtype=np.int64))  # postings stay sorted
                merged = array("q")
                merged.frombytes(a.astype(np.int64).tobytes())
                by_val[v] = merged

    def _pair_rows(self, key: Any, value: Any, n: int) -> np.ndarray:
        """Sorted rows < n with ``meta.get(key) == value``."""
        # rows past the metadata list (the reference allows fewer metadata entries than vectors;
        # persistence pads them with {} on reload) have no keys: get(key) is None
        m_rows = min(n, len(self._rows))
        if not _hashable(value):
            return np.fromiter((i for i in range(m_rows) if isinstance(self._rows[i], dict)
                                and self._rows[i].get(key) == value), dtype=np.int64)
        lst = self._post.get(key, {}).get(value) if _hashable(key) else None
        rows = np.frombuffer(lst, dtype=np.int64) if lst is not None else np.zeros(0, np.int64)
        if value is None:
            # rows without the key also satisfy get(key) == None
            has = np.zeros(n, bool)
            for vals in (self._post.get(key, {}) if _hashable(key) else {}).values():
                a = np.frombuffer(vals, dtype=np.int64)
                has[a[a < n]] = True
            for i in range(m_rows):  # rows holding the key with an unhashable value
                m = self._rows[i]
                if isinstance(m, dict) and key in m and not _hashable(m[key]):
                    has[i] = True
            missing = np.nonzero(~has)[0]
            rows = np.union1d(rows, missing)
        return rows[rows < n]

    # ---- filter operators (service/filter_ops.py) ---------------------------------------------
    def _has_key(self, key: Any, n: int) -> np.ndarray:
        """bool [n]: the row's metadata holds ``key`` (the lock held).  The postings give the rows
        that hold it with a hashable value; a value the postings skip (unhashable, NaN) is found
        only by a pass over the first n metadata dicts, as the ``value is None`` branch of
        ``_pair_rows`` makes: ``$exists`` costs O(n) on the host, once per cached filter."""
        has = np.zeros(n, bool)
        for vals in (self._post.get(key, {}) if _hashable(key) else {}).values():
            a = np.frombuffer(vals, dtype=np.int64)
            has[a[a < n]] = True
        for i in range(min(n, len(self._rows))):  # rows holding the key with a value the postings skip
            m = self._rows[i]
            if isinstance(m, dict) and key in m and not _hashable(m[key]):
                has[i] = True
        return has

    def _numeric_postings(self, key: Any, n: int):
        """(value, rows < n) for every distinct int or float value of ``key`` that is not a bool
        (NaN is held by no posting), from the key's postings (the lock held).  True, 1 and 1.0 --
        and False, 0 and 0.0 -- share one posting, as they are equal and hash alike: the rows of
        those two postings are told apart by the type of the value they hold."""
        by_val = self._post.get(key) if _hashable(key) else None
        for val, lst in (by_val or {}).items():
            if not isinstance(val, (int, float)):
                continue
            a = np.frombuffer(lst, dtype=np.int64)
            a = a[a < n]
            if val == 0 or val == 1:
                keep = [int(r) for r in a.tolist() if not isinstance(self._rows[r].get(key), bool)]
                if not keep:
                    continue
                a = np.asarray(keep, dtype=np.int64)
                val = self._rows[keep[0]].get(key)
            if a.size:
                yield val, a

    def numeric_column(self, key: Any, n: int) -> Tuple[np.ndarray, bool]:
        """(float64 [n], exact): row r's value for ``key`` when it is an int or float that is not a
        bool and not NaN, NaN otherwise ("the row has no value": the column the device's predicate
        masks take, include/vdb.h vdb_index_set_column).  ``exact`` is False when some value v has
        float(v) != v (an int beyond 2^53): the device would then compare a rounded value.  Built
        from the postings of ``key`` alone, O(rows holding it), not by a scan of the dicts."""
        col = np.full(max(int(n), 0), np.nan, dtype=np.float64)
        exact = True
        with self._lock:
            for val, a in self._numeric_postings(key, n):
                try:
                    f = float(val)
                except OverflowError:
                    f, exact = (math.inf if val > 0 else -math.inf), False
                if f != val:
                    exact = False
                col[a] = f
        return col, exact

    def _range_rows(self, key: Any, ops, n: int) -> np.ndarray:
        """Sorted rows < n whose value for ``key`` is a number that every range operator of ``ops``
        holds for, by Python's comparisons over the key's distinct posting values (the lock held)."""
        hits = [a for val, a in self._numeric_postings(key, n) if all(RANGE_OPS[op](val, x) for op, x in ops)]
        return np.sort(np.concatenate(hits)) if hits else np.zeros(0, np.int64)

    def range_rows(self, key: Any, ops, n: int) -> np.ndarray:
        """The host evaluation of a range condition: ``ops`` = [(op, bound)] with op among $gt,
        $gte, $lt, $lte, ANDed; O(distinct values + matching rows)."""
        with self._lock:
            return self._range_rows(key, ops, n)

    def _cond_rows(self, key: Any, ops, n: int) -> np.ndarray:
        """Sorted rows < n for which every operator of a condition on ``key`` holds (the lock held)."""

        def complement(r):
            keep = np.ones(n, bool)
            keep[r] = False
            return np.nonzero(keep)[0]

        def union(values):
            r = np.zeros(0, np.int64)
            for x in values:
                r = np.union1d(r, self._pair_rows(key, x, n))
            return r

        rows = None
        ranges = [(op, x) for op, x in ops if op in RANGE_OPS]
        for op, x in ops:
            if op in RANGE_OPS:
                continue
            if op == "$eq":
                r = self._pair_rows(key, x, n)
            elif op == "$ne":
                r = complement(self._pair_rows(key, x, n))
            elif op == "$in":
                r = union(x)
            elif op == "$nin":
                r = complement(union(x))
            else:  # $exists
                has = self._has_key(key, n)
                r = np.nonzero(has if x else ~has)[0]
            rows = r if rows is None else np.intersect1d(rows, r, assume_unique=True)
        if ranges:
            r = self._range_rows(key, ranges, n)
            rows = r if rows is None else np.intersect1d(rows, r, assume_unique=True)
        return rows if rows is not None else np.arange(n, dtype=np.int64)

    def _match_rows(self, filt: Dict, n: int) -> np.ndarray:
        """Sorted rows < n matching every pair and condition of ``filt`` (the lock held)."""
        rows = None
        for k, v in filt.items():
            pr = self._cond_rows(k, parse_condition(k, v), n) if is_condition(v) else self._pair_rows(k, v, n)
            rows = pr if rows is None else np.intersect1d(rows, pr, assume_unique=True)
            if rows.size == 0:
                break
        if rows is None:
            rows = np.arange(n, dtype=np.int64)
        return rows

    def rows(self, filt: Dict, n: int) -> np.ndarray:
        """The rows < n matching every pair of ``filt``, ascending and unique (int64, the caller's
        own copy): the set ``bitmap`` marks, as the row list the device's row-list search takes
        (include/vdb.h vdb_index_search_rows).  O(matching rows); nothing is cached."""
        with self._lock:
            return np.array(self._match_rows(filt, n), dtype=np.int64)

    def bitmap(self, filt: Dict, n: int) -> Tuple[np.ndarray, int]:
        """(uint32 words of the rows < n matching every pair, match count)."""
        try:  # (condition dicts become tuples; a filter without conditions keys as it always did)
            ck: Optional[Tuple] = (canonical_key(filt), n)
        except TypeError:
            ck = None
        if has_range_ops(filt):
            ck = None  # a range bound usually differs per request: it would only evict the bitmaps that recur
        with self._lock:
            if ck is not None and ck in self._cache:
                self._cache.move_to_end(ck)
                return self._cache[ck]
            rows = self._match_rows(filt, n)
            bits = np.zeros(((n + 31) // 32) * 32, dtype=bool)
            bits[rows] = True
            words = np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)
            out = (words, int(rows.size))
            if ck is not None:
                self._cache[ck] = out
                if len(self._cache) > self.CACHE:
                    self._cache.popitem(last=False)
            return out
