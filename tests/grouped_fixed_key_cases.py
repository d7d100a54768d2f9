"""Plans, tables and filter masks shared by tests/test_grouped_dense_tile_gpu.py and tests/test_grouped_packed_key_cpu.py: grouped aggregates keyed by Utf8
columns of one uniform length each — the shape for which the executor generates k_gagg's fixed-length-key variant (packed LDS key)."""
import numpy as np
import pyarrow as pa

from datafusion_comet_amd import serde as S, tpch

TILE = 512            # rows of one k_gagg tile (R = 2 rows per thread, 256 threads)
WAVE = 64
THRESHOLD = 16        # live lanes per wave row around which the masks are laid out (a quarter of a wave)
ROW_COUNTS = [1, 255, 256, 257, 511, 512, 513, 1023, 1025, 3 * TILE + 17]
CUTOFF = tpch.days(1998, 9, 2)      # Q1's filter: l_shipdate <= CUTOFF

D12, D22, D38 = S.decimal(12, 2), S.decimal(22, 2), S.decimal(38, 6)


def masks(n):
    """name → which rows pass the Filter"""
    i = np.arange(n)
    lanes = lambda t: (i % WAVE) < t
    m = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "threshold-1": lanes(THRESHOLD - 1), "threshold": lanes(THRESHOLD), "threshold+1": lanes(THRESHOLD + 1),
         # dense and sparse tiles in turn within one chunk; within a dense tile one wave row at the threshold
         "alternating": np.where((i // TILE) % 2 == 0, (i % TILE >= WAVE) | lanes(THRESHOLD), i % WAVE == 5),
         "last_dead": i != n - 1, "last_alive": i != n - 2}
    return m


def q1_table(n, mask, seed=None):
    t = tpch.lineitem_q1(n, seed=n if seed is None else seed)
    i = np.arange(n)
    ship = np.where(mask, CUTOFF - (i % 2000), CUTOFF + 1 + (i % 80)).astype(np.int32)
    return t.set_column(6, "l_shipdate", pa.array(ship, pa.int32()).cast(pa.date32()))


def utf8_fixed(codes, length, null=None, alphabet=b"ABCDEFGHIJKLMNOPQRSTUVWXYZ"):
    """a Utf8 column whose every value is `length` bytes long: value k spells codes[k] in base len(alphabet).  A NULL slot keeps its bytes (physically non-zero)."""
    n = len(codes)
    a = np.frombuffer(alphabet, np.uint8)
    data = np.zeros((n, length), np.uint8)
    c = np.asarray(codes, np.int64).copy()
    for j in range(length):
        data[:, j] = a[c % len(a)]
        c //= len(a)
    offs = (np.arange(n + 1, dtype=np.int64) * length).astype(np.int32)
    vb, nulls = None, 0
    if null is not None and null.any():
        vb, nulls = pa.py_buffer(np.packbits(~null, bitorder="little").tobytes()), int(null.sum())
    return pa.Array.from_buffers(pa.utf8(), n, [vb, pa.py_buffer(offs.tobytes()), pa.py_buffer(data.tobytes())], null_count=nulls)


def dec128(vals, p, s):
    return pa.Array.from_buffers(pa.decimal128(p, s), len(vals), [None, pa.py_buffer(b"".join(int(v).to_bytes(16, "little", signed=True) for v in vals))])


KEYED_FIELDS = [S.T_STRING, S.T_STRING, D12, S.T_INT32]


def keyed_plan():
    """HashAgg(Partial, keys = [k1, k2], [sum(v), count(1)]) ← Filter(f = 1) ← Scan[k1 utf8, k2 utf8, v decimal(12,2), f int32]"""
    k1, k2, v, f = (S.col(i, t) for i, t in enumerate(KEYED_FIELDS))
    return S.hash_agg(S.filter_(S.scan(KEYED_FIELDS), S.eq(f, S.lit(1, S.T_INT32))), [k1, k2], [S.sum_(v, D22), S.count(S.lit(1, S.T_INT32))], S.PARTIAL)


KEYED_NUM_OUTPUT_COLS = 2 + 2 + 1


def keyed_table(n, l1, l2, groups, mask, nullable=False, seed=0):
    """`groups` distinct (k1, k2) pairs spread over the rows; with `nullable`, a fifth of each key's slots are NULL (over bytes that stay in place)"""
    rng = np.random.default_rng(seed + 31 * n + groups)
    g = rng.integers(0, groups, n)
    side = 1
    while side * side < groups:
        side += 1
    side = max(side, 2)
    c1, c2 = g % side, g // side
    n1 = (rng.random(n) < 0.2) if nullable else None
    n2 = (rng.random(n) < 0.2) if nullable else None
    v = rng.integers(-10**9, 10**9, n)
    return pa.table([utf8_fixed(c1, l1, n1), utf8_fixed(c2, l2, n2), dec128(v, 12, 2), pa.array(mask.astype(np.int32))], names=["k1", "k2", "v", "f"])


def rows(tbl, nkeys=2):
    if tbl is None:
        return []
    cols = [tbl.column(i).to_pylist() for i in range(tbl.num_columns)]
    return sorted(zip(*cols), key=lambda r: tuple((x is None, "" if x is None else str(x)) for x in r[:nkeys]))


def ansi_plan():
    """sum(a / b), sum(w · 10^19) per (k1, k2) in ANSI mode ← Filter(f = 1) ← Scan: the division raises on b = 0, the product beyond 38 digits"""
    W38 = S.decimal(38, 0)
    fields = [S.T_STRING, S.T_STRING, D12, D12, W38, S.T_INT32]
    k1, k2, a, b, w, f = (S.col(i, t) for i, t in enumerate(fields))
    flt = S.filter_(S.scan(fields), S.eq(f, S.lit(1, S.T_INT32)))
    q = S.math("divide", a, b, S.decimal(27, 15), S.ANSI)
    m = S.math("multiply", w, S.lit(10 ** 19, W38), W38, S.ANSI)
    p = S.project(flt, [k1, k2, q, m])
    return S.hash_agg(p, [S.col(0, S.T_STRING), S.col(1, S.T_STRING)], [S.sum_(S.col(2, S.decimal(27, 15)), S.decimal(37, 15)), S.sum_(S.col(3, W38), W38), S.count(S.lit(1, S.T_INT32))], S.PARTIAL)


def ansi_table(n, offenders, live):
    """rows `offenders` hold b = 0 and w = 10^20; the Filter drops them unless `live`"""
    i = np.arange(n)
    bad = np.zeros(n, bool)
    bad[offenders] = True
    b = np.where(bad, 0, 1 + i % 97)
    w = [10 ** 20 + int(k) if z else int(k) % 1000 for k, z in zip(i, bad)]
    f = np.where(bad & (not live), 0, 1).astype(np.int32)
    return pa.table([utf8_fixed(i % 3, 1), utf8_fixed(i % 2, 1), dec128(1000 + i, 12, 2), dec128(b, 12, 2), dec128(w, 38, 0), pa.array(f)], names=["k1", "k2", "a", "b", "w", "f"])


def sum38_plan():
    fields = [S.T_STRING, S.T_STRING, D38]
    return S.hash_agg(S.scan(fields), [S.col(0, S.T_STRING), S.col(1, S.T_STRING)], [S.sum_(S.col(2, D38), D38), S.count(S.lit(1, S.T_INT32))], S.PARTIAL)


def magnitudes():
    out = {}
    for L in (56, 57, 64, 65):      # bit lengths L − 1, L, L and L + 1
        out["bits%d" % L] = [(1 << (L - 1)) - 1, 1 << (L - 1), (1 << L) - 1, 1 << L]
    # near the 38-digit bound, where the verdict turns: a group's 350 rows of 2e35 fit (7e37), of 4e35 do not (1.4e38)
    out["fits"] = [2 * 10 ** 35]
    out["overflows"] = [4 * 10 ** 35]
    return out


def sum38_table(case, signs, n=700):
    """two groups of decimal(38,6) values cycling through magnitudes()[case]; signs = "mixed": every third value negative"""
    mags = magnitudes()[case]
    i = np.arange(n)
    vals = [mags[k % len(mags)] * (-1 if (signs == "mixed" and k % 3 == 1) else 1) for k in i]
    return pa.table([utf8_fixed(i % 2, 1), utf8_fixed(np.zeros(n, np.int64), 1), dec128(vals, 38, 6)], names=["k1", "k2", "c"])
