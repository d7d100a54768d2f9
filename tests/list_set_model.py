"""Spark's ArrayUnion, ArrayIntersect, ArrayExcept and ArraysOverlap over Python lists — the model the set-function tests hold the engine to.

Lists, elements and values as in tests/list_fn_model.py: a list is a Python list or None (a NULL list), an element is a value or None (a NULL element), str is
compared as its UTF-8 bytes.  Every result is NULL when either argument is; NULL elements count as one value in union, intersect and except."""
from tests.list_fn_model import _key, array_distinct


def _has(arr, v):
    """value equality, NULL equal to NULL"""
    return any(w is None for w in arr) if v is None else any(w is not None and _key(w) == _key(v) for w in arr)


def array_union(a, b):
    """distinct(a ++ b): first occurrences, a's before b's"""
    return None if a is None or b is None else array_distinct(a + b)


def array_intersect(a, b):
    """the distinct elements of a, in a's order, that occur in b"""
    return None if a is None or b is None else [v for v in array_distinct(a) if _has(b, v)]


def array_except(a, b):
    """the distinct elements of a, in a's order, that do not occur in b"""
    return None if a is None or b is None else [v for v in array_distinct(a) if not _has(b, v)]


def arrays_overlap(a, b):
    """three-valued: true when a non-NULL value stands in both; else NULL when a side holds a NULL element — unless a side is empty; else false"""
    if a is None or b is None:
        return None
    if not a or not b:
        return False
    if any(v is not None and _has(b, v) for v in a):
        return True
    return None if (None in a or None in b) else False
