"""Filter operators: the condition language of ``filter_metadata``.

A value of ``filter_metadata`` that is a non-empty dict whose keys all start with ``$`` is a
CONDITION on that key; its operators are ANDed, as the keys of the filter are.  Every other value
-- a dict with any non-``$`` key included -- keeps the equality meaning ``meta.get(key) == value``
(service/metadata_index.py).

    $eq: x        meta.get(key) == x          (so ``$eq: None`` also matches rows lacking the key)
    $ne: x        the complement of $eq
    $in: [x, ..]  the union of $eq over the list
    $nin: [..]    the complement of $in
    $exists: b    (key in meta) == b
    $gt $gte $lt $lte: x    the row has the key with an int or float value that is not a bool and
                  not NaN, and Python's own comparison with x holds (int against float is exact)

``row_matches`` is that definition over one metadata dict.  The posting operators are answered from
the postings on the host (MetadataIndex); the range operators of a key fold into one interval,
which the device evaluates as one clause of include/vdb.h vdb_index_filter_mask when the key's
column and the bounds are exact in fp64, and the host otherwise (the store's ``_filter_masks``).
Top-level ``$or`` and nesting are not part of the language.
"""
from __future__ import annotations

import math
import operator
from typing import Any, Dict, List, Optional, Tuple

POSTING_OPS = ("$eq", "$ne", "$in", "$nin", "$exists")
RANGE_OPS = {"$gt": operator.gt, "$gte": operator.ge, "$lt": operator.lt, "$lte": operator.le}
ALL_OPS = POSTING_OPS + tuple(RANGE_OPS)


class FilterError(ValueError):
    """A malformed condition: an unknown ``$`` operator or a bad operand."""


def is_condition(value: Any) -> bool:
    """A non-empty dict whose keys all start with ``$``."""
    return (isinstance(value, dict) and len(value) > 0
            and all(isinstance(k, str) and k.startswith("$") for k in value))


def is_number(v: Any) -> bool:
    """An int or float that is not a bool and not NaN: what a range operator compares."""
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        return False
    return not (isinstance(v, float) and math.isnan(v))


def parse_condition(key: Any, cond: Dict) -> List[Tuple[str, Any]]:
    """The (op, operand) pairs of a condition, checked: an unknown ``$`` key or a bad operand
    raises ValueError."""
    out = []
    for op, x in cond.items():
        if op not in ALL_OPS:
            raise FilterError(f"unknown filter operator {op!r} on key {key!r}; known: {', '.join(ALL_OPS)}")
        if op in RANGE_OPS:
            if not is_number(x):
                raise FilterError(f"{op} on key {key!r} takes an int or float that is not a bool and not NaN, "
                                 f"got {x!r}")
        elif op in ("$in", "$nin"):
            if not isinstance(x, (list, tuple)):
                raise FilterError(f"{op} on key {key!r} takes a list of values, got {x!r}")
            x = tuple(x)
        elif op == "$exists":
            if not isinstance(x, bool):
                raise FilterError(f"$exists on key {key!r} takes true or false, got {x!r}")
        out.append((op, x))
    return out


def split_filter(filt: Optional[Dict]) -> Tuple[Dict, Dict[Any, List[Tuple[str, Any]]]]:
    """(plain pairs, conditions: key -> [(op, operand)]) of a filter, every condition checked."""
    plain: Dict = {}
    conds: Dict[Any, List[Tuple[str, Any]]] = {}
    for k, v in (filt or {}).items():
        if is_condition(v):
            conds[k] = parse_condition(k, v)
        else:
            plain[k] = v
    return plain, conds


def has_conditions(filt: Optional[Dict]) -> bool:
    return bool(filt) and any(is_condition(v) for v in filt.values())


def range_ops(ops: List[Tuple[str, Any]]) -> List[Tuple[str, Any]]:
    return [(op, x) for op, x in ops if op in RANGE_OPS]


def posting_ops(ops: List[Tuple[str, Any]]) -> List[Tuple[str, Any]]:
    return [(op, x) for op, x in ops if op not in RANGE_OPS]


def fold_range(ops: List[Tuple[str, Any]]) -> Tuple[Any, bool, Any, bool]:
    """The range operators of one key as one interval (lo, lo_inclusive, hi, hi_inclusive): the
    largest lower and the smallest upper bound, the exclusive one winning a tie.  The bounds stay
    the Python numbers they were (compared exactly); no lower / upper bound is -inf / +inf,
    inclusive, which every value that is a number passes."""
    lo, lo_incl, hi, hi_incl = -math.inf, True, math.inf, True
    for op, x in ops:
        if op == "$gt" and x >= lo:
            lo, lo_incl = x, False
        elif op == "$gte" and x > lo:
            lo, lo_incl = x, True
        elif op == "$lt" and x <= hi:
            hi, hi_incl = x, False
        elif op == "$lte" and x < hi:
            hi, hi_incl = x, True
    return lo, lo_incl, hi, hi_incl


def in_interval(v: Any, iv: Tuple[Any, bool, Any, bool]) -> bool:
    """A number against a folded interval, by Python's comparisons."""
    lo, lo_incl, hi, hi_incl = iv
    return (v >= lo if lo_incl else v > lo) and (v <= hi if hi_incl else v < hi)


def float_exact(x: Any) -> bool:
    """float(x) == x: the bound or value survives the conversion to fp64 unchanged."""
    try:
        return float(x) == x
    except OverflowError:
        return False


def _op_holds(meta: Dict, key: Any, op: str, x: Any) -> bool:
    if op == "$eq":
        return meta.get(key) == x
    if op == "$ne":
        return not meta.get(key) == x
    if op == "$in":
        return any(meta.get(key) == y for y in x)
    if op == "$nin":
        return not any(meta.get(key) == y for y in x)
    if op == "$exists":
        return (key in meta) == x
    v = meta.get(key) if key in meta else None
    return is_number(v) and bool(RANGE_OPS[op](v, x))


def compile_filter(filt: Optional[Dict]):
    """``filt`` parsed and checked once -> a function of one row's metadata: the definition.  (A
    row without a metadata dict holds no key.)"""
    plain, conds = split_filter(filt)

    def matches(meta: Any) -> bool:
        m = meta if isinstance(meta, dict) else {}
        for k, v in plain.items():
            if not m.get(k) == v:
                return False
        for k, ops in conds.items():
            for op, x in ops:
                if not _op_holds(m, k, op, x):
                    return False
        return True

    return matches


def row_matches(meta: Any, filt: Optional[Dict]) -> bool:
    """Does one row's metadata match ``filt``?  (``compile_filter`` for many rows.)"""
    return compile_filter(filt)(meta)


def has_range_ops(filt: Optional[Dict]) -> bool:
    """Some condition of ``filt`` carries a range operator (nothing is checked)."""
    return bool(filt) and any(is_condition(v) and any(op in RANGE_OPS for op in v) for v in filt.values())


def _canon(v: Any) -> Any:
    if is_condition(v):  # (only the lists of $in / $nin become tuples: as values, [1] and (1,) differ)
        return ("$cond",) + tuple(sorted(((op, tuple(x) if op in ("$in", "$nin") and isinstance(x, list) else x)
                                          for op, x in v.items()), key=lambda ox: ox[0]))
    return v


def canonical_key(filt: Dict):
    """A hashable key equal for filters holding the same pairs and conditions (condition dicts
    and their lists become tuples); raises TypeError when a value is unhashable."""
    key = tuple(sorted(((k, _canon(v)) for k, v in filt.items()), key=lambda kv: repr(kv[0])))
    hash(key)
    return key
