"""Spark's runtime Bloom filters on the GPU: bloom_filter_agg (Partial / PartialMerge / Final) as an operator over its materialised child and might_contain
inside the fused kernels, against the pure-Python model of tests/bloom_model.py (the reference's rules restated; its known answers are pinned by
tests/test_bloom_filter_cpu.py).  Everything is compared exactly: filter bytes, and per-row TRUE / FALSE / NULL — which implies no false negative.

Sizes: 64 and 192 bits (one and three words; 192 is no power of two: the remainder is a real one), 2^16 bits (the largest filter built per block in LDS),
2^16 + 64 (the smallest built in global memory, no power of two) and 2^23 (Spark's default runtime filter).  numItems is chosen so that k = 1 and k = 7."""
import functools
import struct

import numpy as np
import pyarrow as pa
import pytest

from datafusion_comet_amd import native, serde as S
from tests import bloom_model as M

pytestmark = pytest.mark.gpu
I32, I64, BIN = S.T_INT32, S.T_INT64, S.T_BINARY

SIZES = [64, 192, 1 << 16, (1 << 16) + 64, 1 << 23]
N = 100_003


def items_for(bits, k):
    """numItems with optimal_k(numItems, bits) == k"""
    items = bits if k == 1 else max(1, round(bits * 0.6931471805599453 / k))
    assert M.optimal_k(items, bits) == k, (bits, k, items)
    return items


SHAPES = [(bits, version, k) for bits in SIZES for version in (1, 2) for k in (1, 7)]
SHAPE_IDS = [f"{b}bits-V{v}-k{k}" for b, v, k in SHAPES]


@functools.lru_cache(maxsize=None)
def data():
    """N longs (full range, some small, duplicates), a third of them NULL"""
    rng = np.random.default_rng(20261019)
    v = rng.integers(-2**63, 2**63 - 1, N, dtype=np.int64)
    v[::7] = rng.integers(-1000, 1000, len(v[::7]))
    valid = rng.random(N) >= 1 / 3
    v32 = rng.integers(-2**31, 2**31 - 1, N, dtype=np.int64)
    return v, valid, v32


def column(values, valid, typ=pa.int64()):
    return pa.array(values, typ, mask=None if valid is None else ~valid)


def run(plan, tables, ncols, batch_rows=8192, subqueries=None):
    ins = [native.HostInput.from_table(t, batch_rows) for t in tables]
    out = native.execute_to_table(ins, ncols, plan.encode(), batch_size=0, subqueries=subqueries)
    return pa.Table.from_batches(out) if out else None


def agg_plan(mode, child_type, bits, version, k, child=None):
    e = child if child is not None else S.col(0, child_type)
    return S.hash_agg(S.scan([child_type]), [], [S.bloom_filter_agg(e, items_for(bits, k), bits, version)], mode)


def one_binary(t):
    assert t is not None and t.num_rows == 1 and t.num_columns == 1
    assert t.schema.field(0).type in (pa.binary(), pa.large_binary()), t.schema
    return t.column(0).to_pylist()[0]


def model_state(values, valid, bits, version, k):
    f = M.Filter(version, k, bits // 64)
    return M.put_all_np(f, values, valid)


# --------------------------------------------------------------------------- build

@pytest.mark.parametrize("bits,version,k", SHAPES, ids=SHAPE_IDS)
def test_partial_state_equals_the_model_for_every_row_count_and_batching(built, bits, version, k):
    v, valid, v32 = data()
    for n in (0, 1, 255, 257, N):
        want = model_state(v[:n], valid[:n], bits, version, k).serialize()
        t = pa.table({"a": column(v[:n], valid[:n])})
        for batch_rows in ((8192,) if n < 1000 else (N, 1000)):
            got = one_binary(run(agg_plan(S.PARTIAL, I64, bits, version, k), [t], 1, batch_rows))
            assert got == want, (n, batch_rows, len(got), len(want))
    # all rows NULL, and no rows: a state that is not NULL, with all-zero words
    empty = M.Filter(version, k, bits // 64).serialize()
    t = pa.table({"a": column(v[:257], np.zeros(257, dtype=bool))})
    assert one_binary(run(agg_plan(S.PARTIAL, I64, bits, version, k), [t], 1)) == empty
    assert model_state(v[:0], valid[:0], bits, version, k).serialize() == empty
    # the same as Int32: sign-extended to a long in the kernel's load
    for n in (257, N):
        want = model_state(v32[:n], valid[:n], bits, version, k).serialize()
        t = pa.table({"a": column(v32[:n], valid[:n], pa.int32())})
        assert one_binary(run(agg_plan(S.PARTIAL, I32, bits, version, k), [t], 1, 1000)) == want, n


@pytest.mark.parametrize("bits,version,k", [(192, 1, 7), (1 << 16, 2, 7), ((1 << 16) + 64, 1, 1), (1 << 23, 2, 7)], ids=lambda x: str(x))
def test_final_and_partial_merge(built, bits, version, k):
    v, valid, _ = data()
    parts = [model_state(v[a:b], valid[a:b], bits, version, k) for a, b in ((0, 300), (300, 301), (0, 0))]      # (one of them empty)
    states = pa.table({"s": pa.array([p.serialize() for p in parts], pa.binary())})
    want = M.Filter(version, k, bits // 64)
    for p in parts:
        want.merge(p)
    assert one_binary(run(agg_plan(S.FINAL, BIN, bits, version, k, child=S.col(0, I64)), [states], 1)) == want.serialize() == want.final()
    # PartialMerge re-emits the state; chained: PartialMerge over (PartialMerge's output ++ one more state) → Final
    pm = one_binary(run(agg_plan(S.PARTIAL_MERGE, BIN, bits, version, k, child=S.col(0, I64)), [states.slice(0, 2)], 1))
    assert pm == M.Filter.parse(parts[0].serialize()).merge(parts[1]).serialize()
    more = model_state(v[500:900], valid[500:900], bits, version, k)
    chained = pa.table({"s": pa.array([pm, more.serialize()], pa.binary())})
    pm2 = one_binary(run(agg_plan(S.PARTIAL_MERGE, BIN, bits, version, k, child=S.col(0, I64)), [chained], 1))
    fin = one_binary(run(agg_plan(S.FINAL, BIN, bits, version, k, child=S.col(0, I64)), [pa.table({"s": pa.array([pm2], pa.binary())})], 1))
    assert fin == want.merge(more).serialize()
    # only empty states: PartialMerge keeps the all-zero state, Final is NULL
    empties = pa.table({"s": pa.array([parts[2].serialize()] * 2, pa.binary())})
    assert one_binary(run(agg_plan(S.PARTIAL_MERGE, BIN, bits, version, k, child=S.col(0, I64)), [empties], 1)) == parts[2].serialize()
    assert one_binary(run(agg_plan(S.FINAL, BIN, bits, version, k, child=S.col(0, I64)), [empties], 1)) is None
    assert parts[2].final() is None


def test_merge_refuses_states_that_do_not_match_by_the_references_messages(built):
    bits, k = 192, 7
    good = M.Filter(2, k, 3).put_all([1, 2, 3])
    cases = [(M.Filter(1, k, 3).serialize(), "version mismatch"), (M.Filter(2, 5, 3).serialize(), "num_hash_functions mismatch"),
             (M.Filter(2, k, 3, seed=9).serialize(), "seed mismatch"), (M.Filter(2, k, 4).serialize(), "num_words mismatch"),
             (good.serialize()[:-1], "truncated bit array")]
    for bad, why in cases:
        states = pa.table({"s": pa.array([good.serialize(), bad], pa.binary())})
        for mode in (S.FINAL, S.PARTIAL_MERGE):
            with pytest.raises(native.CometNativeException, match="BloomFilter merge: " + why):
                run(agg_plan(mode, BIN, bits, 2, k, child=S.col(0, I64)), [states], 1)


# --------------------------------------------------------------------------- probe

@functools.lru_cache(maxsize=None)
def probe_values():
    """N probe longs, a fifth of them NULL; the first half are values of data() (present in the filters below wherever they were valid there)"""
    rng = np.random.default_rng(7)
    v, _, _ = data()
    p = np.concatenate([v[:N // 2], rng.integers(-2**63, 2**63 - 1, N - N // 2, dtype=np.int64)])
    valid = rng.random(N) >= 0.2
    other = rng.integers(-50, 50, N).astype(np.int32)
    return p, valid, other


@functools.lru_cache(maxsize=None)
def probe_filter(bits, version, k):
    """a filter holding as many of data()'s values as leave about half of its bits clear"""
    v, valid, _ = data()
    n = max(1, min(N // 2, bits // (2 * k)))
    return model_state(v[:n], valid[:n], bits, version, k)


def want_probe(f, p, valid):
    hit = M.might_contain_np(f, p)
    return [bool(h) if ok else None for h, ok in zip(hit, valid)]


def probe_table():
    p, valid, other = probe_values()
    return pa.table({"v": column(p, valid), "o": pa.array(other, pa.int32())})


@pytest.mark.parametrize("bits,version,k", SHAPES, ids=SHAPE_IDS)
def test_might_contain_as_projection_and_as_filter(built, bits, version, k):
    p, valid, _ = probe_values()
    f = probe_filter(bits, version, k)
    want = want_probe(f, p, valid)
    assert any(w is True for w in want) and (bits == 64 or any(w is False for w in want))
    mc = S.bloom_filter_might_contain(S.lit(f.serialize(), BIN), S.col(0, I64))
    got = run(S.project(S.scan([I64, I32]), [mc]), [probe_table()], 1)
    assert got.column(0).to_pylist() == want
    got = run(S.filter_(S.scan([I64, I32]), mc), [probe_table()], 2)
    assert (got.column(0).to_pylist() if got is not None else []) == [int(x) for x, w in zip(p, want) if w]
    # every value that was put is found
    v, dvalid, _ = data()
    n = max(1, min(N // 2, bits // (2 * k)))
    assert all(w for w, ok, dv in zip(want[:n], valid[:n], dvalid[:n]) if ok and dv)


def test_might_contain_under_and_or_not_with_other_predicates(built):
    p, valid, other = probe_values()
    f = probe_filter(1 << 16, 2, 7)
    want = want_probe(f, p, valid)
    mc = S.bloom_filter_might_contain(S.lit(f.serialize(), BIN), S.col(0, I64))
    gt = S.gt(S.col(1, I32), S.lit(0, I32))
    got = run(S.filter_(S.scan([I64, I32]), S.and_(gt, mc)), [probe_table()], 2)
    assert got.column(0).to_pylist() == [int(x) for x, w, o in zip(p, want, other) if w and o > 0]
    got = run(S.filter_(S.scan([I64, I32]), S.or_(gt, S.not_(mc))), [probe_table()], 2)
    keep = [i for i in range(N) if other[i] > 0 or want[i] is False]
    assert got.column(1).to_pylist() == [int(other[i]) for i in keep] and got.column(0).to_pylist() == [int(p[i]) if valid[i] else None for i in keep]


def xxhash64_np(values, seed=42):
    import xxhash
    return np.array([xxhash.xxh64_intdigest(struct.pack("<q", int(x)), seed=seed) for x in values], dtype=np.uint64).view(np.int64)


def test_the_shape_spark_sends_filter_over_xxhash64_then_count(built):
    """Filter(might_contain(filter, xxhash64(fk, 42))) above the scan, feeding count(*): the probe-side chain of InjectRuntimeFilter"""
    rng = np.random.default_rng(11)
    keys = rng.integers(0, 5000, 20_011).astype(np.int64)
    kvalid = rng.random(len(keys)) >= 0.1
    small = np.arange(0, 5000, 9, dtype=np.int64)
    f = M.put_all_np(M.Filter(1, 6, 8192 // 64), xxhash64_np(small))
    hit = M.might_contain_np(f, xxhash64_np(keys))
    want = [int(x) for x, h, ok in zip(keys, hit, kvalid) if ok and h]
    assert set(small.tolist()) & set(keys[kvalid].tolist()) <= set(want) and len(want) < int(kvalid.sum())
    xx = S.scalar_func("xxhash64", [S.col(0, I64), S.lit(42, I64)], I64)
    t = pa.table({"k": column(keys, kvalid)})
    # a NULL key hashes to the seed (xxhash64 is never NULL): Spark's plan carries isnotnull(fk) beside it
    pred = S.and_(S.is_not_null(S.col(0, I64)), S.bloom_filter_might_contain(S.lit(f.serialize(), BIN), xx))
    got = run(S.filter_(S.scan([I64]), pred), [t], 1)
    assert got.column(0).to_pylist() == want
    got = run(S.hash_agg(S.filter_(S.scan([I64]), pred), [], [S.count(S.col(0, I64))], S.PARTIAL), [t], 1, 1000)
    assert got.column(0).to_pylist() == [len(want)]


def test_as_the_probe_side_filter_of_a_hash_join(built):
    rng = np.random.default_rng(13)
    fk = rng.integers(0, 3000, 30_007).astype(np.int64)
    pay = np.arange(len(fk), dtype=np.int64)
    dim = np.arange(0, 3000, 17, dtype=np.int64)
    f = M.put_all_np(M.Filter(2, 6, 4096 // 64), dim)
    probe = pa.table({"fk": pa.array(fk), "pay": pa.array(pay)})
    build = pa.table({"k": pa.array(dim)})
    mc = S.bloom_filter_might_contain(S.lit(f.serialize(), BIN), S.col(0, I64))

    def join(left):
        return S.hash_join(left, S.scan([I64]), [S.col(0, I64)], [S.col(0, I64)], S.INNER, build_side=S.BUILD_RIGHT)
    filtered = run(join(S.filter_(S.scan([I64, I64]), mc)), [probe, build], 3)
    plain = run(join(S.scan([I64, I64])), [probe, build], 3)
    rows = lambda t: sorted(zip(*(t.column(i).to_pylist() for i in range(3))))      # noqa: E731
    assert rows(filtered) == rows(plain) == sorted((int(a), int(b), int(a)) for a, b in zip(fk, pay) if a % 17 == 0)


def test_null_filters_two_filters_and_the_fifth(built):
    p, valid, _ = probe_values()
    t = probe_table().slice(0, 4099)
    v = S.col(0, I64)
    # a NULL filter — literal, and subquery resolved to NULL — is NULL for every row; as a predicate no row survives
    for filt, sub in ((S.lit(None, BIN), None), (S.subquery(3, BIN), {3: None})):
        mc = S.bloom_filter_might_contain(filt, v)
        assert run(S.project(S.scan([I64, I32]), [mc]), [t], 1, subqueries=sub).column(0).to_pylist() == [None] * 4099
        got = run(S.filter_(S.scan([I64, I32]), mc), [t], 2, subqueries=sub)
        assert got is None or got.num_rows == 0
    # two filters in one predicate: a literal and a subquery, different shapes
    f1, f2 = probe_filter(192, 1, 7), probe_filter((1 << 16) + 64, 2, 1)
    w1, w2 = want_probe(f1, p[:4099], valid[:4099]), want_probe(f2, p[:4099], valid[:4099])
    pred = S.and_(S.bloom_filter_might_contain(S.lit(f1.serialize(), BIN), v), S.bloom_filter_might_contain(S.subquery(1, BIN), v))
    got = run(S.filter_(S.scan([I64, I32]), pred), [t], 2, subqueries={1: f2.serialize()})
    assert got.column(0).to_pylist() == [int(x) for x, a, b in zip(p, w1, w2) if a and b]
    # the same plan bytes with another filter behind the subquery: the other answer (and, the source being filter-independent, the same kernels)
    f3 = probe_filter(1 << 16, 1, 7)
    w3 = want_probe(f3, p[:4099], valid[:4099])
    got = run(S.filter_(S.scan([I64, I32]), pred), [t], 2, subqueries={1: f3.serialize()})
    assert got.column(0).to_pylist() == [int(x) for x, a, b in zip(p, w1, w3) if a and b]
    # untrusted bytes behind a subquery are refused by name before anything runs
    with pytest.raises(native.CometNativeException, match="might_contain.*version 3"):
        run(S.filter_(S.scan([I64, I32]), pred), [t], 2, subqueries={1: struct.pack(">iii", 3, 1, 1) + bytes(8)})
    # a fifth probe in one chain is refused by name
    five = None
    for i in range(5):
        mc = S.bloom_filter_might_contain(S.lit(f1.serialize(), BIN), S.math("add", v, S.lit(i, I64), I64))
        five = mc if five is None else S.and_(five, mc)
    with pytest.raises(native.CometNativeException, match="might_contain: more than 4"):
        run(S.filter_(S.scan([I64, I32]), five), [t], 2)


def test_end_to_end_build_side_then_probe_side(built):
    """plan A: Partial → Final of bloom_filter_agg(xxhash64(k)) on the small side; its bytes go in through comet_plan_set_subquery; plan B filters the large side"""
    rng = np.random.default_rng(17)
    small = rng.choice(100_000, 2_000, replace=False).astype(np.int64)
    large = rng.integers(0, 100_000, 50_021).astype(np.int64)
    num_items, num_bits = 2_000, 1 << 17
    xx = S.scalar_func("xxhash64", [S.col(0, I64), S.lit(42, I64)], I64)
    agg = S.bloom_filter_agg(xx, num_items, num_bits, 2)
    halves = [pa.table({"k": pa.array(small[:1200])}), pa.table({"k": pa.array(small[1200:])})]
    states = [one_binary(run(S.hash_agg(S.scan([I64]), [], [agg], S.PARTIAL), [h], 1)) for h in halves]
    final = one_binary(run(S.hash_agg(S.scan([BIN]), [], [agg], S.FINAL), [pa.table({"s": pa.array(states, pa.binary())})], 1))
    model = M.put_all_np(M.Filter.for_agg(num_items, num_bits, 2), xxhash64_np(small))
    assert final == model.serialize()
    plan_b = S.filter_(S.scan([I64]), S.bloom_filter_might_contain(S.subquery(0, BIN), xx))
    got = run(plan_b, [pa.table({"k": pa.array(large)})], 1, subqueries={0: final})
    hit = M.might_contain_np(model, xxhash64_np(large))
    assert got.column(0).to_pylist() == [int(x) for x, h in zip(large, hit) if h]
    assert set(small.tolist()) & set(large.tolist()) <= set(got.column(0).to_pylist())
