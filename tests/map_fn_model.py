"""Spark's GetMapValue / element_at over a map, MapKeys, MapValues, MapEntries and MapContainsKey over Python values — the model the map-function tests hold the
engine to (Spark's GetMapValueUtil; tests/test_map_fn_cpu.py pins it against Spark's answers for the reference's SQL tests).

A map is a list of (key, value) pairs in entry order, or None (a NULL map); a value is a value or None (a NULL value); a key is never None.  Keys of one map
are of one kind: bool, int (integers, dates and timestamps as their numbers, decimals as their unscaled value) or str (Utf8: equal when their bytes are)."""


def map_extract(m, k):
    """m[k] and element_at(m, k): the value of the FIRST entry, in entry order, whose key equals k — NULL where that value is NULL; NULL for a NULL map, a NULL
    key and when no entry matches.  Never an error, in any ANSI mode (what arrives is map_extract wrapped in a ListExtract that does not fail)."""
    if m is None or k is None:
        return None
    for key, value in m:
        if type(key) is type(k) and key == k:      # (True == 1 in Python: a Boolean key is not an integer key)
            return value
    return None


def map_keys(m):
    """List<key>, NULL for a NULL map; the keys as they stand, in entry order"""
    return None if m is None else [k for k, _ in m]


def map_values(m):
    """List<value>, NULL for a NULL map; NULL elements where the values are NULL"""
    return None if m is None else [v for _, v in m]


def map_entries(m):
    """List<Struct<key, value>>, NULL for a NULL map"""
    return None if m is None else [{"key": k, "value": v} for k, v in m]


def map_contains_key(m, k):
    """Spark rewrites it to array_contains(map_keys(m), k): NULL for a NULL map or key, else whether a key equals k (keys are never NULL, so never NULL for
    another reason)"""
    if m is None or k is None:
        return None
    return any(type(key) is type(k) and key == k for key, _ in m)


def size(m):
    """size(m) under spark.sql.legacy.sizeOfNull (what the native function answers): -1 for a NULL map"""
    return -1 if m is None else len(m)
