"""Spark's SortArray, ArrayDistinct, ArrayMin, ArrayMax and ArrayPosition over Python lists — the model the list-function tests hold the engine to.

A list is a Python list or None (a NULL list); an element is a value or None (a NULL element).  Values of one list are of one kind: bool, int (integers, dates
and timestamps as their numbers, decimals as their unscaled value), or bytes / str (Utf8; str is compared as its UTF-8 bytes: unsigned bytes, a proper prefix
first — which is Python's own order of bytes objects)."""


def _key(v):
    return v.encode() if isinstance(v, str) else v


def sort_array(arr, ascending=True, nulls_last=None):
    """array_sort(arr, 'ASC' | 'DESC', 'NULLS FIRST' | 'NULLS LAST').  Spark's sort_array(arr, asc) puts NULL elements first when ascending and last when
    descending (nulls_last=None: that rule); the engine takes the null rank as a parameter of its own.  Equal values keep their order."""
    if arr is None:
        return None
    if nulls_last is None:
        nulls_last = not ascending
    nulls = [v for v in arr if v is None]
    vals = sorted((v for v in arr if v is not None), key=_key, reverse=not ascending)      # (sorted is stable under reverse too)
    return vals + nulls if nulls_last else nulls + vals


def array_distinct(arr):
    """the first occurrence of every value in its original position order; NULL elements count as one value"""
    if arr is None:
        return None
    seen, saw_null, out = set(), False, []
    for v in arr:
        if v is None:
            if not saw_null:
                out.append(None)
            saw_null = True
        elif _key(v) not in seen:
            seen.add(_key(v))
            out.append(v)
    return out


def _extreme(arr, pick):
    if arr is None:
        return None
    vals = [v for v in arr if v is not None]
    return pick(vals, key=_key) if vals else None


def array_min(arr):
    """the least non-NULL element; NULL for a NULL list, an empty list and a list of NULL elements only"""
    return _extreme(arr, min)


def array_max(arr):
    return _extreme(arr, max)


def array_position(arr, key):
    """the one-based position of the first non-NULL element equal to the key, 0 when there is none; NULL when the list or the key is NULL"""
    if arr is None or key is None:
        return None
    for i, v in enumerate(arr):
        if v is not None and _key(v) == _key(key):
            return i + 1
    return 0
