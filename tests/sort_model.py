"""TEST INFRASTRUCTURE: a vectorised model of Sort / TopK (SortExec with fetch and skip) in plain numpy, and the key tables the sort tests share.

The oracle's Sort is a Python comparison sort: exact, but far too slow for the 300 000-row shapes at which the device's sort takes its other paths.  This
model answers the same question through np.lexsort: every key becomes a NULL rank (0 or 1 by NULLS FIRST / LAST) and the dense rank of an order-preserving
value (integers as they are, floats by their IEEE totalOrder integer, decimals as Python ints, strings as bytes); DESC negates the value rank, never the NULL
rank; the row index is the last key, so the order is total — the oracle's sort is stable, so the two agree row for row.  tests/test_sort_model_cpu.py pins
the model to the oracle; the GPU tests then compare the device with the model.

A key is a column index of the table, or an Arrow array of as many rows (a computed key the test evaluated itself: substring(s, 1, 3), a + b)."""
import numpy as np
import pyarrow as pa


def _one_chunk(a):
    if isinstance(a, pa.ChunkedArray):
        a = a.combine_chunks() if a.num_chunks != 1 else a.chunk(0)
    return a


def _values(a):
    """(valid, order-preserving values) of an Arrow array: an int64 array, or an object array of Python ints / bytes; what a NULL slot holds is unspecified"""
    a = _one_chunk(a)
    n, t = len(a), a.type
    valid = np.ones(n, bool) if a.null_count == 0 else np.asarray(a.is_valid().to_numpy(zero_copy_only=False), bool)
    if pa.types.is_boolean(t):
        return valid, np.asarray(a.fill_null(False).to_numpy(zero_copy_only=False), bool).astype(np.int64)
    if pa.types.is_floating(t):
        # IEEE totalOrder: the bits as a signed integer; a negative one has every bit but the sign inverted (−NaN < −inf < … < −0.0 < +0.0 < … < +inf < +NaN)
        it = np.int64 if t == pa.float64() else np.int32
        bits = np.frombuffer(a.buffers()[1], dtype=it)[a.offset:a.offset + n].astype(np.int64)
        return valid, np.where(bits < 0, bits ^ np.int64(np.iinfo(it).max), bits)
    if pa.types.is_decimal(t):
        raw = np.frombuffer(a.buffers()[1], dtype=np.dtype([("lo", "<u8"), ("hi", "<i8")]))[a.offset:a.offset + n]
        out = np.empty(n, object)
        for i in range(n):
            out[i] = (int(raw["hi"][i]) << 64) | int(raw["lo"][i])
        return valid, out
    if pa.types.is_string(t) or pa.types.is_binary(t) or pa.types.is_large_string(t):
        out = np.empty(n, object)
        for i, v in enumerate(a.to_pylist()):
            out[i] = b"" if v is None else (v.encode() if isinstance(v, str) else bytes(v))      # bytes compare unsigned, prefixes first (UTF8String.compareTo)
        return valid, out
    if pa.types.is_date32(t):
        a = a.cast(pa.int32())
    elif pa.types.is_timestamp(t) or pa.types.is_date64(t):
        a = a.cast(pa.int64())
    elif not pa.types.is_integer(t):
        raise TypeError("sort_model: no order for %s" % t)
    return valid, np.asarray(a.fill_null(0).to_numpy(zero_copy_only=False)).astype(np.int64)


def _key_array(table, key):
    return _one_chunk(table.column(key)) if isinstance(key, (int, np.integer)) else _one_chunk(key)


def rank_keys(table, orders):
    """(n, 2·keys) int64: per key its NULL rank and the (DESC: negated) dense rank of its value, 0 where NULL.  Rows compare under the sort like their rows of
    this matrix compare lexicographically, and two rows hold equal keys (NULL = NULL, −0.0 ≠ 0.0, NaNs by payload) exactly when their rows here are equal."""
    n = table.num_rows
    out = np.zeros((n, 2 * len(orders)), np.int64)
    for k, (key, desc, nulls_last) in enumerate(orders):
        valid, vals = _values(_key_array(table, key))
        assert len(vals) == n
        rank = np.zeros(n, np.int64)
        if valid.any():
            _, inv = np.unique(vals[valid], return_inverse=True)
            rank[valid] = inv.reshape(-1) + 1
        out[:, 2 * k] = np.where(valid, 0 if nulls_last else 1, 1 if nulls_last else 0)
        out[:, 2 * k + 1] = -rank if desc else rank
    return out


def expected_order(table, orders, fetch=None, skip=0):
    """row indices of `table` in the order Sort(orders, fetch, skip) delivers them; ties in row order.  orders: (key, descending, nulls_last)"""
    n = table.num_rows
    r = rank_keys(table, orders)
    order = np.lexsort([np.arange(n)] + [r[:, c] for c in range(r.shape[1] - 1, -1, -1)]) if n else np.zeros(0, np.int64)
    if fetch is not None and fetch >= 0:
        order = order[:fetch]                                  # fetch counts from the first row, then skip (SortExec under a GlobalLimit)
    if skip:
        order = order[skip:]
    return order.astype(np.int64)


def _canon(a):
    """a column as a list that compares bit for bit: floats by their bits (NaN payloads, the sign of zero), everything else by value; None for NULL"""
    a = _one_chunk(a)
    if pa.types.is_floating(a.type):
        it = np.int64 if a.type == pa.float64() else np.int32
        bits = np.frombuffer(a.buffers()[1], dtype=it)[a.offset:a.offset + len(a)]
        ok = np.ones(len(a), bool) if a.null_count == 0 else np.asarray(a.is_valid().to_numpy(zero_copy_only=False), bool)
        return [int(b) if o else None for b, o in zip(bits, ok)]
    if pa.types.is_decimal(a.type):      # (the two words, not decimal.Decimal objects: a 300 000-row payload column stays cheap)
        raw = np.frombuffer(a.buffers()[1], dtype=np.dtype([("lo", "<u8"), ("hi", "<i8")]))[a.offset:a.offset + len(a)]
        ok = np.ones(len(a), bool) if a.null_count == 0 else np.asarray(a.is_valid().to_numpy(zero_copy_only=False), bool)
        return [(l, h) if o else None for l, h, o in zip(raw["lo"].tolist(), raw["hi"].tolist(), ok.tolist())]
    if pa.types.is_date32(a.type) or pa.types.is_timestamp(a.type):      # (days and microseconds beyond what datetime holds)
        a = a.cast(pa.int32() if pa.types.is_date32(a.type) else pa.int64())
    return a.to_pylist()


def assert_same_rows(got, table, rows, cols=None):
    """`got` (a table, or None for no batch) holds exactly rows `rows` of `table`, in that order, bit for bit, in every column (or in `cols`)"""
    if len(rows) == 0:
        assert got is None or got.num_rows == 0, got
        return
    assert got is not None and got.num_rows == len(rows), (None if got is None else got.num_rows, len(rows))
    want = table.take(pa.array(rows, pa.int64()))
    for c in (range(table.num_columns) if cols is None else cols):
        assert got.column(c).type == want.column(c).type, (c, got.column(c).type, want.column(c).type)
        g, w = _canon(got.column(c)), _canon(want.column(c))
        if g != w:
            bad = next(i for i in range(len(g)) if g[i] != w[i])
            raise AssertionError("column %d differs first at output row %d (input row %d): got %r, want %r" % (c, bad, rows[bad], g[bad], w[bad]))


def check_sorted(got, table, orders, fetch, skip, id_col):
    """A sort whose keys have ties may deliver tied rows in any order, and a fetch (or a skip) may cut a run of tied rows anywhere.  With `id_col` a column
    of unique ids that the sort carries along:
      1. the key columns of `got` equal the model's, row for row (as values for column keys, and as key ranks for every key);
      2. for every key value strictly inside the output — not the first one when rows were skipped, not the last one — the ids are the model's, as a set;
      3. for the last key value (and the first, under a skip) the ids are distinct input rows of that key, as many as the model has.
    Every output row falls under 1 and under 2 or 3."""
    model = expected_order(table, orders, fetch, skip)
    if len(model) == 0:
        assert got is None or got.num_rows == 0, got
        return
    assert got is not None and got.num_rows == len(model), (None if got is None else got.num_rows, len(model))
    ids = np.asarray(_one_chunk(table.column(id_col)).to_numpy(zero_copy_only=False))
    by_id = np.argsort(ids, kind="stable")
    assert len(np.unique(ids)) == len(ids), "id_col is not unique"
    gid = np.asarray(_one_chunk(got.column(id_col)).to_numpy(zero_copy_only=False))
    pos = np.searchsorted(ids[by_id], gid)
    assert (pos < len(ids)).all() and (ids[by_id][np.minimum(pos, len(ids) - 1)] == gid).all(), "an output id is not an input id"
    grow = by_id[pos]                                       # the input row of every output row
    assert len(np.unique(grow)) == len(grow), "an input row came out twice"
    r = rank_keys(table, orders)
    assert (r[grow] == r[model]).all(), "key ranks differ first at output row %d" % int(np.argmax((r[grow] != r[model]).any(axis=1)))
    assert_same_rows(got, table, model, cols=[k for k, _, _ in orders if isinstance(k, (int, np.integer))])      # … and the values that came out are those keys
    same_as_last = (r[model] == r[model[-1]]).all(axis=1)
    open_end = same_as_last if fetch is not None and fetch >= 0 else np.zeros(len(model), bool)
    if skip:
        open_end = open_end | (r[model] == r[model[0]]).all(axis=1)
    assert sorted(grow[~open_end].tolist()) == sorted(model[~open_end].tolist()), "rows of a key value that is wholly inside the output differ from the model's"
    # the cut runs: distinct (above) input rows of that very key, as many as the model has
    for edge in ([model[-1]] if open_end.any() else []) + ([model[0]] if skip else []):
        run_out = (r[model] == r[edge]).all(axis=1)
        of_key = np.flatnonzero((r == r[edge]).all(axis=1))
        assert np.isin(grow[run_out], of_key).all() and int(run_out.sum()) == int((r[grow] == r[edge]).all(axis=1).sum()), "the run of tied rows a fetch / skip cuts holds foreign rows"


# --------------------------------------------------------------------------- the key types the sort tests share

def _with_edges(edges, fill, n, rng, null_rate=0.08):
    """n values: every edge value twice (so that equal keys exist), random fill behind them; → (values, mask) with NULLs only among the fill and two at the front"""
    vals = list(edges) + list(edges) + list(fill[:max(0, n - 2 * len(edges))])
    vals = vals[:n]
    mask = np.zeros(len(vals), bool)
    mask[2 * len(edges):] = rng.random(len(vals) - 2 * len(edges)) < null_rate
    perm = rng.permutation(len(vals))
    return [vals[i] for i in perm], mask[perm]


def _dec_array(ints, mask, p, s):
    raw = np.zeros(len(ints), np.dtype([("lo", "<u8"), ("hi", "<i8")]))
    for i, v in enumerate(ints):
        raw["lo"][i], raw["hi"][i] = int(v) & 0xFFFFFFFFFFFFFFFF, int(v) >> 64
    vb = pa.py_buffer(np.packbits(~mask, bitorder="little").tobytes()) if mask.any() else None
    return pa.Array.from_buffers(pa.decimal128(p, s), len(ints), [vb, pa.py_buffer(raw.tobytes())], null_count=int(mask.sum()))


def _float_array(bits, mask, wide):
    """a Float32 / Float64 array from raw bit patterns (NaN payloads survive)"""
    raw = np.array(bits, np.uint64 if wide else np.uint32)
    vb = pa.py_buffer(np.packbits(~mask, bitorder="little").tobytes()) if mask.any() else None
    return pa.Array.from_buffers(pa.float64() if wide else pa.float32(), len(raw), [vb, pa.py_buffer(raw.tobytes())], null_count=int(mask.sum()))


def key_cases(S, n=400, seed=7):
    """One case per sortable key type: {name, table, fields, key (the sort expression), model (what sort_model takes for it), width (value bytes of its key;
    None: a Utf8 column, padded to its longest value + 4), g / id (columns of a low-cardinality nullable Int32 and of the row number)}."""
    rng = np.random.default_rng(seed)
    cases = []

    def add(name, arrays, fields, key, model, width):
        g = pa.array(rng.integers(0, 3, n).astype(np.int32), mask=rng.random(n) < 0.1)
        cols = list(arrays) + [g, pa.array(np.arange(n, dtype=np.int64))]
        fl = list(fields) + [S.T_INT32, S.T_INT64]
        cases.append(dict(name=name, table=pa.table(cols, names=["c%d" % i for i in range(len(cols))]), fields=fl, key=key(fl) if callable(key) else key,
                          model=model, width=width, g=len(cols) - 2, id=len(cols) - 1))

    v, m = _with_edges([True, False], (rng.random(n) < 0.5).tolist(), n, rng)
    add("bool", [pa.array(v, pa.bool_(), mask=m)], [S.T_BOOL], S.col(0, S.T_BOOL), 0, 1)
    ts_ntz = S.DataType(S.TIMESTAMP_NTZ)
    for name, npt, pat, st, bits in (("int8", np.int8, pa.int8(), S.T_INT8, 8), ("int16", np.int16, pa.int16(), S.T_INT16, 16), ("int32", np.int32, pa.int32(), S.T_INT32, 32),
                                     ("int64", np.int64, pa.int64(), S.T_INT64, 64), ("date", np.int32, pa.date32(), S.T_DATE, 32), ("timestamp", np.int64, pa.timestamp("us", tz="UTC"), S.T_TIMESTAMP, 64),
                                     ("timestamp_ntz", np.int64, pa.timestamp("us"), ts_ntz, 64)):
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        edges = [lo, hi, -1, 0, 1, lo + 1, hi - 1, 255, 256, -256, -257][:11 if bits > 8 else 7]
        fill = rng.integers(lo, hi, n, dtype=np.int64, endpoint=True).tolist()
        v, m = _with_edges(edges, fill, n, rng)
        base = pa.array(np.array(v, np.int64).astype(npt), mask=m)
        add(name, [base.cast(pat) if base.type != pat else base], [st], S.col(0, st), 0, bits // 8)
    for name, wide, st in (("float32", False, S.T_FLOAT), ("float64", True, S.T_DOUBLE)):
        sign = 1 << (63 if wide else 31)
        inf, qnan, mx = (0x7FF0000000000000, 0x7FF8000000000000, 0x7FEFFFFFFFFFFFFF) if wide else (0x7F800000, 0x7FC00000, 0x7F7FFFFF)
        pos = [0, 1, mx, inf, qnan, qnan | 5, inf | 1]                 # +0, smallest subnormal, max, inf, two quiet NaN payloads, a signalling NaN
        edges = pos + [p | sign for p in pos]
        ft = np.float64 if wide else np.float32
        fill = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(ft).view(np.uint64 if wide else np.uint32).tolist()
        v, m = _with_edges(edges, fill, n, rng)
        add(name, [_float_array(v, m, wide)], [st], S.col(0, st), 0, 8 if wide else 4)
    for p, s in ((9, 2), (18, 0), (20, 4), (38, 10)):
        top = 10 ** p - 1
        edges = [top, -top, 0, 1, -1, top - 1, 1 - top]
        if p > 18:      # values that differ only in the high word, and only in the low word
            edges += [1 << 64, (1 << 64) + 1, 2 << 64, -(1 << 64), -(1 << 64) - 1, (1 << 64) - 1, (3 << 64) + 7 if p > 20 else (5 << 64) + 7, (4 << 64) + 7 if p > 20 else (5 << 64) + 8]
            edges = [e for e in edges if abs(e) <= top]
        # half of the fill over the whole range, half small (where only the low bytes vary)
        fill = [int(x) * int(y) % (2 * top + 1) - top if i & 1 else int(x) % 2001 - 1000 for i, (x, y) in enumerate(zip(rng.integers(0, 1 << 62, n), rng.integers(0, 1 << 62, n)))]
        v, m = _with_edges(edges, fill, n, rng)
        st = S.decimal(p, s)
        add("decimal(%d,%d)" % (p, s), [_dec_array(v, m, p, s)], [st], S.col(0, st), 0, 16)
    words = ["", "a", "a\x00", "ab", "abc", "abd", "b", "é", "éa", "日本", "日本語", "\U0001F600", "￿", "z" * 300, "Zebra", "zebra"]
    fill = ["%s%d" % (words[int(i)][:8], int(j)) for i, j in zip(rng.integers(0, len(words), n), rng.integers(0, 40, n))]
    v, m = _with_edges(words, fill, n, rng)
    add("utf8", [pa.array(v, pa.string(), mask=m)], [S.T_STRING], S.col(0, S.T_STRING), 0, None)
    short = ["", "a", "ab", "abc", "abcd", "abd", "fifteen-bytes-15", "fifteen-bytes-1", "fifteen-bytes-2x", "日本語x", "éééé", "ab\x00", "ab\x00\x00"]
    fill = ["%s%d" % (short[int(i)][:5], int(j)) for i, j in zip(rng.integers(0, len(short), n), rng.integers(0, 2000, n))]
    v, m = _with_edges(short, fill, n, rng)
    for take in (3, 15):      # substring(s, 1, take): results of 0 … take characters, at most 15 bytes (the packed computed-string key)
        sub = pa.array([None if mm else x[:take] for x, mm in zip(v, m)], pa.string())
        assert max(len(x.encode()) for x in sub.to_pylist() if x is not None) == (9 if take == 3 else 15)
        add("substring(s,1,%d)" % take, [pa.array(v, pa.string(), mask=m)], [S.T_STRING],
            S.scalar_func("substring", [S.col(0, S.T_STRING), S.lit(1, S.T_INT32), S.lit(take, S.T_INT32)], S.T_STRING), sub, 16)
    a = rng.integers(-(1 << 40), 1 << 40, n)
    b = rng.integers(-(1 << 40), 1 << 40, n)
    a[:6], b[:6] = [0, 1, -1, 5, (1 << 40), -(1 << 40)], [0, -1, 0, -5, (1 << 40), -(1 << 40)]
    ma, mb = rng.random(n) < 0.06, rng.random(n) < 0.06
    ma[:6] = mb[:6] = False
    add("a+b", [pa.array(a, pa.int64(), mask=ma), pa.array(b, pa.int64(), mask=mb)], [S.T_INT64, S.T_INT64],
        S.math("add", S.col(0, S.T_INT64), S.col(1, S.T_INT64), S.T_INT64), pa.array(a + b, pa.int64(), mask=ma | mb), 8)
    return cases


# --------------------------------------------------------------------------- the executor's path, read off the data

_WIDTH = {pa.bool_(): 1, pa.int8(): 1, pa.int16(): 2, pa.int32(): 4, pa.date32(): 4, pa.int64(): 8, pa.float32(): 4, pa.float64(): 8}


def key_bytes(table, orders):
    """(n, W) uint8: the order-preserving key bytes of fixed-width keys, written down independently of the generator — per key one NULL byte (NULLS FIRST: NULL 0,
    value 1; NULLS LAST: NULL 1, value 0), then the value big-endian with its sign bit flipped (floats: their totalOrder integer), inverted for DESC, zero for NULL"""
    n = table.num_rows
    out = []
    for key, desc, nulls_last in orders:
        a = _key_array(table, key)
        valid, vals = _values(a)
        w = 16 if pa.types.is_decimal(a.type) else 8 if pa.types.is_timestamp(a.type) else _WIDTH[a.type]
        out.append(np.where(valid, 0 if nulls_last else 1, 1 if nulls_last else 0).astype(np.uint8).reshape(n, 1))
        if w == 16:
            b = np.frombuffer(b"".join(((int(v) + (1 << 127)) & ((1 << 128) - 1)).to_bytes(16, "big") for v in vals), np.uint8).reshape(n, 16).copy()
        else:
            u = vals.astype(np.int64).view(np.uint64) if pa.types.is_boolean(a.type) else (vals.astype(np.int64) + np.int64(1 << (8 * w - 1)) if w < 8 else vals.astype(np.int64) ^ np.int64(-1 << 63)).view(np.uint64)
            b = np.stack([((u >> np.uint64(8 * (w - 1 - k))) & np.uint64(255)).astype(np.uint8) for k in range(w)], axis=1)
        if desc:
            b = ~b
        b[~valid] = 0
        out.append(b)
    return np.concatenate(out, axis=1)


def sort_path(K, fetch=None, skip=0):
    """What sort_table (csrc/exec_sort.cpp) does with rows whose key bytes are K, as the four counters it keeps — None when it sorts nothing.  A plane "varies"
    when it holds more than one distinct byte; the TopK branch runs when fetch·8 < rows, one radix-select pass per varying plane from the most significant one
    while more than max(4096, rows still needed) candidates are left; what is left goes to the one-workgroup sort when it is at most 4096 rows and at most 16
    planes vary, else through one LSD radix pass per varying plane."""
    n, W = K.shape
    fetch = -1 if fetch is None else fetch
    keep = min(n, fetch) if fetch >= 0 else n
    if n == 0 or keep - min(max(0, skip), n) <= 0:
        return None
    varies = [bool(K[:, b].min() != K[:, b].max()) for b in range(W)]
    ns, passes = n, 0
    if fetch >= 0 and keep * 8 < n:
        cand, need, nsure = np.arange(n), keep, 0
        for b in range(W):
            if not len(cand) > max(4096, need):
                break
            if not varies[b]:
                continue
            h = np.bincount(K[cand, b], minlength=256)
            below, dstar = 0, 255
            for d in range(256):
                if below + h[d] >= need:
                    dstar = d
                    break
                below += int(h[d])
            cand = cand[K[cand, b] == dstar]
            nsure, need, passes = nsure + below, need - below, passes + 1
        if passes:
            ns = nsure + len(cand)
    small = ns <= 4096 and sum(varies) <= 16
    return {"sort_select_passes": passes, "sort_small_sorts": 1 if small else 0, "sort_radix_passes": 0 if small else sum(varies), "sort_rows_sorted": int(ns)}
