"""Spark's runtime Bloom filters without a GPU: the model of tests/bloom_model.py against the reference's murmur3 vectors and four known serializations; the host
diagnostics (the code of csrc/device/bloom.hpp, compiled for the host) against the model; what createPlan accepts and refuses; and that the generated kernel
text does not depend on the filter.

Known answers: k = 4, seed 0, values [1, 42, 1000000, −7, −2^63, 2^63 − 1] into 256 and 192 bits, V1 and V2 — computed by a model of the rules whose murmur3
passes the reference's vectors (tests/golden/reference_kats.json): an independent restatement to agree with, not the output of a reference binary."""
import json
import math
import os
import struct

import numpy as np
import pytest

from datafusion_comet_amd import native, serde as S
from tests import bloom_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32, I64, BIN = S.T_INT32, S.T_INT64, S.T_BINARY
VALUES = [1, 42, 1000000, -7, -2**63, 2**63 - 1]
KNOWN = {(1, 256): "0000000100000004000000040010400001000282600000008800001009204002100200400000000040400482",
         (1, 192): "000000010000000400000003012040008902065060104002504000820800000000000082",
         (2, 256): "00000002000000040000000000000004040d0000460000800042000000000b2000000000200004000008100400084100",
         (2, 192): "00000002000000040000000000000003004a000422000900004d0000040846200400100040000180"}


def items_for_k4(bits):
    items = round(bits * math.log(2.0) / 4)
    assert M.optimal_k(items, bits) == 4
    return items


def test_the_models_murmur3_is_the_references():
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kats.json")))["murmur3"]["i64"]
    assert [M.murmur3_long(v, 42) for v in kat["values"]] == kat["expected"]
    assert M.murmur3_long_np(np.array(kat["values"], dtype=np.int64), 42).tolist() == kat["expected"]


@pytest.mark.parametrize("version,bits", sorted(KNOWN))
def test_known_serializations(built, version, bits):
    want = bytes.fromhex(KNOWN[(version, bits)])
    assert M.Filter(version, 4, bits // 64).put_all(VALUES).serialize() == want
    assert native.spark_bloom_build(VALUES, items_for_k4(bits), bits, version) == want
    assert native.spark_bloom_build(VALUES + [None], items_for_k4(bits), bits, version) == want      # a NULL input is ignored
    assert all(native.spark_bloom_might_contain(want, v) is True for v in VALUES)
    assert M.Filter.parse(want).serialize() == want


def test_the_vectorised_model_is_the_scalar_one():
    rng = np.random.default_rng(3)
    v = rng.integers(-2**63, 2**63 - 1, 1500, dtype=np.int64)
    for version in (1, 2):
        for bits, k in ((64, 1), (192, 7), (1 << 16, 7), ((1 << 16) + 64, 3)):
            assert (M.indices_np(version, k, 0, bits, v) == np.array([M.indices(version, k, 0, bits, int(x)) for x in v])).all()
            f, g = M.Filter(version, k, bits // 64), M.Filter(version, k, bits // 64)
            M.put_all_np(f, v[:400])
            g.put_all(int(x) for x in v[:400])
            assert f.words == g.words and M.might_contain_np(f, v).tolist() == [g.might_contain(int(x)) for x in v]


@pytest.mark.parametrize("version", [0, 1, 2])
@pytest.mark.parametrize("bits,items", [(1 << 16, 6000), (192, 19), ((1 << 16) + 64, 65600), (4096, 4096 * 3)])
def test_host_diagnostics_agree_with_the_model_bit_for_bit(built, version, bits, items):
    rng = np.random.default_rng(bits + version)
    ins = rng.integers(-2**63, 2**63 - 1, 10_000, dtype=np.int64)
    ins[::5] = rng.integers(-100, 100, len(ins[::5]))
    n_in = max(1, min(len(ins), bits // 16))      # (leave clear bits, so that the probes below see both answers)
    model = M.put_all_np(M.Filter.for_agg(items, bits, version), ins[:n_in])
    got = native.spark_bloom_build([int(x) for x in ins[:n_in]], items, bits, version)
    assert got == model.serialize()
    assert all(native.spark_bloom_might_contain(got, int(x)) for x in ins[:n_in])
    others = rng.integers(-2**63, 2**63 - 1, 10_000, dtype=np.int64)
    want = M.might_contain_np(model, others).tolist()
    assert [native.spark_bloom_might_contain(got, int(x)) for x in others] == want
    assert not all(want) and (bits > 4096 or any(want))      # false positives included


def test_malformed_filters_are_rejected(built):
    good = M.Filter(1, 3, 2).put_all([5]).serialize()
    v2 = M.Filter(2, 3, 2).put_all([5]).serialize()

    def v1(version, k, nwords, words=None):
        return struct.pack(">iii", version, k, nwords) + (bytes(8 * max(nwords, 0)) if words is None else words)
    bad = {"version 3": v1(3, 3, 2), "numHashFunctions 0": v1(1, 0, 2), "numHashFunctions 256": v1(1, 256, 2), "numWords 0": v1(1, 3, 0), "truncated": good[:-1],
           "empty": b"", "truncated ": v2[:14], "too large": v1(1, 3, 1 << 25, b"")}
    assert native.spark_bloom_might_contain(good, 5) is True and native.spark_bloom_might_contain(v2, 5) is True
    for why, b in bad.items():
        assert native.spark_bloom_might_contain(b, 5) is None, why
        # … and by name where a plan carries them
        ok, msg = native.check_plan(S.filter_(S.scan([I64]), S.bloom_filter_might_contain(S.lit(b, BIN), S.col(0, I64))).encode())
        assert not ok and "might_contain" in msg and why.strip() in msg, (why, msg)
    assert native.spark_bloom_might_contain(v1(1, 255, 1), 5) is False      # k = 255 is the largest accepted


def test_round_half_away_from_zero(built):
    """k = max(1, round(numBits / numItems · ln 2)) with f64::round.  For x in 1, 2, 6, 40: (numBits, numItems) pairs, found by search, whose quotient · ln 2 lies within
    1e-9 below and within 1e-9 above x.5: the first gives x, the second x + 1 (the quotient is computed here as the engine computes it: one division, one product)"""
    ln2 = math.log(2.0)
    bits = np.arange(1 << 23, 1 << 24, dtype=np.int64)
    for x in (1, 2, 6, 40):
        for side in (-1, 1):
            items0 = np.floor(bits * ln2 / (x + 0.5)).astype(np.int64)
            found = None
            for items in (items0, items0 + 1):
                d = bits / items * ln2 - (x + 0.5)
                at = np.nonzero((d * side > 0) & (np.abs(d) < 1e-9))[0]
                if len(at):
                    found = (int(bits[at[0]]), int(items[at[0]]))
                    break
            assert found, (x, side)
            nbits, nitems = found
            q = nbits / nitems * ln2
            assert 0 < (q - (x + 0.5)) * side < 1e-9
            want = x + 1 if side > 0 else x
            assert M.optimal_k(nitems, nbits) == want
            got = native.spark_bloom_build([], nitems, nbits, 1)
            assert struct.unpack(">i", got[4:8])[0] == want, (nbits, nitems, q)
    assert M.round_half_away(2.5) == 3 and M.round_half_away(0.5) == 1 and M.round_half_away(0.49999999999999994) == 0
    assert struct.unpack(">i", native.spark_bloom_build([], 1000, 64, 1)[4:8])[0] == 1      # max(1, round(0.044))


def agg(child, items=1000, bits=8192, version=0, **kw):
    return S.bloom_filter_agg(child, items, bits, version, **kw)


def test_check_plan_accepts_the_two_shapes_spark_sends(built):
    xx = S.scalar_func("xxhash64", [S.col(0, I64), S.lit(42, I64)], I64)
    for plan in (S.hash_agg(S.scan([I64]), [], [agg(xx)], S.PARTIAL), S.hash_agg(S.scan([BIN]), [], [agg(xx)], S.FINAL), S.hash_agg(S.scan([BIN]), [], [agg(xx)], S.PARTIAL_MERGE),
                 S.hash_agg(S.scan([I32]), [], [agg(S.col(0, I32), version=2)], S.PARTIAL),
                 S.filter_(S.scan([I64]), S.bloom_filter_might_contain(S.subquery(7, BIN), xx)),
                 S.filter_(S.scan([I64, I32]), S.and_(S.gt(S.col(1, I32), S.lit(0, I32)), S.or_(S.not_(S.bloom_filter_might_contain(S.subquery(7, BIN), xx)), S.is_null(S.col(0, I64))))),
                 S.project(S.scan([I64]), [S.bloom_filter_might_contain(S.lit(None, BIN), S.col(0, I64))]),
                 S.hash_join(S.filter_(S.scan([I64]), S.bloom_filter_might_contain(S.subquery(1, BIN), xx)), S.scan([I64]), [S.col(0, I64)], [S.col(0, I64)], S.INNER, build_side=S.BUILD_RIGHT)):
        ok, msg = native.check_plan(plan.encode())
        assert ok, msg
    assert "bloom_filter_agg (Partial): V1, 6 hash function(s), 8192 bits" in native.check_plan(S.hash_agg(S.scan([I64]), [], [agg(xx)], S.PARTIAL).encode())[1]


def test_check_plan_refuses_the_rest_by_name(built):
    c, xx = S.col(0, I64), S.scalar_func("xxhash64", [S.col(0, I64), S.lit(42, I64)], I64)
    good = M.Filter(1, 3, 2).serialize()
    refused = [
        (S.hash_agg(S.scan([I64]), [c], [agg(xx)]), "grouped"), (S.hash_agg(S.scan([I64]), [], [agg(xx), S.count(c)]), "mixed"),
        (S.hash_agg(S.scan([I64]), [], [agg(xx, filter=S.gt(c, S.lit(1, I64)))]), "FILTER"), (S.hash_agg(S.scan([S.T_STRING]), [], [agg(S.col(0, S.T_STRING))]), "Utf8"),
        (S.hash_agg(S.scan([I64]), [], [agg(xx, items=0)]), "numItems"), (S.hash_agg(S.scan([I64]), [], [agg(xx, items=-5)]), "numItems"),
        (S.hash_agg(S.scan([I64]), [], [agg(xx, bits=0)]), "numBits"), (S.hash_agg(S.scan([I64]), [], [agg(xx, items=10**6, bits=2**31 - 1)]), "2^31"),
        (S.hash_agg(S.scan([I64]), [], [agg(xx, items=2**32 + 5, bits=2**32)]), "numBits"),      # (truncated to i32: 0 bits)
        (S.hash_agg(S.scan([I64]), [], [agg(xx, items=1, bits=8192)]), "255"), (S.hash_agg(S.scan([S.T_DOUBLE]), [], [agg(S.col(0, S.T_DOUBLE))]), "Float64"),
        (S.hash_agg(S.scan([I64]), [], [agg(xx)], S.FINAL), "Binary state")]
    for plan, why in refused:
        ok, msg = native.check_plan(plan.encode())
        assert not ok and "bloom_filter_agg" in msg and why in msg, (why, msg)
    mc = S.bloom_filter_might_contain
    five = None
    for i in range(5):
        e = mc(S.lit(good, BIN), S.math("add", c, S.lit(i, I64), I64))
        five = e if five is None else S.and_(five, e)
    wide = S.scan([I64] * 24)
    refused = [(S.project(S.scan([I64, BIN]), [mc(S.col(1, BIN), c)]), "Binary literal or a Binary scalar subquery"), (S.project(S.scan([I64]), [mc(S.lit("ab", S.T_STRING), c)]), "Binary literal"),
               (S.project(S.scan([I64]), [mc(S.subquery(1, S.T_STRING), c)]), "Binary"), (S.project(S.scan([I32]), [mc(S.lit(good, BIN), S.col(0, I32))]), "Int64"),
               (S.filter_(S.scan([I64]), five), "more than 4"), (S.project(S.filter_(wide, mc(S.lit(good, BIN), c)), [c]), "slot")]
    for plan, why in refused:
        ok, msg = native.check_plan(plan.encode())
        assert not ok and "might_contain" in msg and why in msg, (why, msg)
    four = S.filter_(S.scan([I64]), five.children[0])
    assert native.check_plan(four.encode())[0]


def test_generated_text_does_not_depend_on_the_filter(built):
    """two plans whose filter literals differ in content, size, k and version generate the same source (one compiled module, one JIT-cache entry); a NULL
    filter is a plan-time fact and may differ"""
    xx = S.scalar_func("xxhash64", [S.col(0, I64), S.lit(42, I64)], I64)

    def plan(filt):
        return S.project(S.filter_(S.scan([I64, I32]), S.and_(S.gt(S.col(1, I32), S.lit(3, I32)), S.bloom_filter_might_contain(filt, xx))), [S.col(0, I64)])
    a = M.Filter(1, 3, 4).put_all(range(100)).serialize()
    b = M.Filter(2, 7, 1 << 10).put_all(range(50, 90)).serialize()
    texts = [native.plan_codegen(plan(S.lit(f, BIN)).encode(), [True, False])["source"] for f in (a, b)]
    assert texts[0] == texts[1] and "bloom_might_contain((const u64*)prm.in[23].data" in texts[0]
    assert native.plan_codegen(plan(S.subquery(4, BIN)).encode(), [True, False])["source"] == texts[0]
    null = native.plan_codegen(plan(S.lit(None, BIN)).encode(), [True, False])["source"]
    assert "bloom_might_contain" not in null
    # … and the join's probe kernels likewise
    def jplan(f):
        return S.hash_join(S.filter_(S.scan([I64]), S.bloom_filter_might_contain(S.lit(f, BIN), xx)), S.scan([I64]), [S.col(0, I64)], [S.col(0, I64)], S.INNER, build_side=S.BUILD_RIGHT)
    ja, jb = (native.plan_codegen(jplan(f).encode(), [False, False])["source"] for f in (a, b))
    assert ja == jb and "bloom_might_contain" in ja
