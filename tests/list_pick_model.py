"""Spark's ArrayRemove, array_compact, Slice, Reverse of an array and ArrayJoin over Python lists — the model the one-list pick tests hold the engine to.

Lists, elements and values as in tests/list_fn_model.py: a list is a Python list or None (a NULL list), an element is a value or None (a NULL element), str is
compared as its UTF-8 bytes.  Every result is NULL when the list is."""
from tests.list_fn_model import _key


def array_remove(arr, key):
    """the list without its non-NULL elements equal to the key; NULL elements stay; NULL when the key is"""
    if arr is None or key is None:
        return None
    return [v for v in arr if v is None or _key(v) != _key(key)]


def array_compact(arr):
    """the list without its NULL elements"""
    return None if arr is None else [v for v in arr if v is not None]


def slice_(arr, start, length):
    """Spark's slice for start != 0 and length >= 0 (it raises otherwise): one-based from the front, negative from the end; a start before the beginning or past
    the end gives the empty list, a length past the end is clamped"""
    assert start != 0 and length >= 0
    if arr is None:
        return None
    n = len(arr)
    z = start - 1 if start > 0 else start + n
    if z < 0 or z >= n or length == 0:
        return []
    return arr[z:z + min(length, n - z)]


def array_reverse(arr):
    return None if arr is None else arr[::-1]


def array_join(arr, delimiter, replacement=None):
    """the non-NULL elements joined by the delimiter; with a replacement every NULL element is written as it.  An empty list gives the empty string, never NULL"""
    if arr is None:
        return None
    pieces = [v if v is not None else replacement for v in arr if v is not None or replacement is not None]
    return delimiter.join(pieces)
