"""regexp_replace(str, pattern, replacement, 'g') (strings.scala:545-587 sends it under spark.comet.expression.RegExpReplace.allowIncompatible; DataFusion's
regexp_replace with the g flag = the crate's Regex::replace_all) as a Utf8 column DERIVED from the source table: two passes of rx_replace per row on the
device (regex_kernels.hip: the source tests/test_regexp_replace_cpu.py walks on the host) — lengths, prefix sum, bytes — then a column like any other to the
chain: an output, a comparison's operand, the subject of length.  The oracle does not evaluate regexp_replace: the expectation is `_want` below, the rule
itself (the text between find_iter's matches, the replacement expanded per match, the rest) over oracle.find_iter_like_the_crate."""
import re

import numpy as np
import pyarrow as pa
import pytest

from datafusion_comet_amd import native, serde as S

pytestmark = pytest.mark.gpu
STR, I32 = S.T_STRING, S.T_INT32
s, k = S.col(0, STR), S.col(1, I32)
R = S.regexp_replace

WORDS = ["", "100-200", "abc", "phone 123-456-7890", "a,b,c,,", ",,,", "x", "one, two ,three", "k1=v1;k2=v2;;k3", "日本,語テ,キスト", "naïve  café   au lait", "foo123bar456baz", "2024-06-30",
         "a" * 50 + "," + "b" * 60, "axxbéc", " leading and trailing "]

_memo = {}


def _segments(rep):
    """Captures::expand's reading of a replacement: literal text | group number"""
    out = []
    for m in re.finditer(r"\$\$|\$\{(\d+)\}|\$(\d+)|\$|[^$]+", rep):
        out.append("$" if m.group() in ("$$", "$") else int(m.group(1) or m.group(2)) if m.group().startswith("$") else m.group())
    return out


def _want(pattern, rep, v):
    if v is None:
        return None
    key = (pattern, rep, v)
    if key not in _memo:
        from oracle import oracle as O
        rx, segs, out, last = O.crate_pattern_to_python(pattern), _segments(rep), [], 0
        for m in O.find_iter_like_the_crate(rx, v):
            out.append(v[last:m.start()])
            out.extend(g if isinstance(g, str) else (m.group(g) or "") for g in segs)
            last = m.end()
        _memo[key] = "".join(out) + v[last:]
    return _memo[key]


def _table(n, seed=31, words=WORDS):
    """rows [100, 100 + n) of a longer table: the column arrives with an Arrow offset"""
    rng = np.random.default_rng(seed)
    w = np.array(words, dtype=object)
    t = pa.table({"s": pa.array(w[rng.integers(0, len(w), n + 150)], pa.utf8(), mask=rng.random(n + 150) < 0.1), "k": pa.array(rng.integers(0, 100, n + 150), pa.int32())})
    return t.slice(100, n)


def _run(plan, table, ncols, **kw):
    return pa.Table.from_batches(native.execute_to_table([native.HostInput.from_table(table)], ncols, plan.encode(), batch_size=0, **kw))


def _check(cases, table, source=None, keep=None):
    """cases: (pattern, replacement) per output column, behind them s and k passed through; keep: the rows the source's Filter keeps"""
    src = source if source is not None else S.scan([STR, I32])
    plan = S.project(src, [R(s, p, r) for p, r in cases] + [s, k])
    ok, msg = native.check_plan(plan.encode())
    assert ok, msg
    got = _run(plan, table, len(cases) + 2)
    vals, ks = table.column(0).to_pylist(), table.column(1).to_pylist()
    rows = [i for i in range(len(vals)) if keep is None or keep(ks[i])]
    for c, (p, r) in enumerate(cases):
        assert got.column(c).to_pylist() == [_want(p, r, vals[i]) for i in rows], (p, r)
    assert got.column(len(cases)).to_pylist() == [vals[i] for i in rows] and got.column(len(cases) + 1).to_pylist() == [ks[i] for i in rows]
    return got


CASES = [("[^0-9]", ""), (",", " , "), ("x*", "-"), (r"(\w+)=(\w*)", "${2}<-$1 $$"), ("[^0-9]", ""), ("", "·"), (r"\s+", " ")]


def test_the_references_vectors(built):
    t = pa.table({"s": pa.array(["100-200", "abc", "", "phone 123-456-7890", None]), "k": pa.array(np.arange(5, dtype=np.int32))})
    got = _check([(r"(\d+)", "X"), (r"(\d+)-(\d+)", "$2-$1")], t)
    assert got.column(0).to_pylist() == ["X-X", "abc", "", "phone X-X-X", None]
    assert got.column(1).to_pylist() == ["200-100", "abc", "", "phone 456-123-7890", None]


def test_deletion_growth_empty_matches_and_templates(built):
    t = _table(30_000)
    assert t.column(0).chunk(0).offset == 100
    got = _check(CASES, t)
    assert got.column(0).null_count == t.column(0).null_count > 0
    out0 = got.column(0).to_pylist()
    assert "" in out0 and "100200" in out0      # deletion empties some rows
    # the same expression twice is one derived column
    plan = S.project(S.scan([STR, I32]), [R(s, p, r) for p, r in CASES])
    assert native.plan_codegen(plan.encode(), [True, False])["derived"] == len(set(CASES))


def test_below_a_filter_and_with_no_rows(built):
    t = _table(40_000, 32)
    got = _check(CASES[:4], t, S.filter_(S.scan([STR, I32]), S.lt(k, S.lit(20, I32))), keep=lambda v: v < 20)
    assert 0 < got.num_rows < t.num_rows
    none = S.filter_(S.scan([STR, I32]), S.lt(k, S.lit(-1, I32)))
    assert native.execute_to_table([native.HostInput.from_table(t)], 1, S.project(none, [R(s, ",", ";")]).encode(), batch_size=0) == []


def test_as_an_operand(built):
    t = _table(20_000, 33)
    vals = t.column(0).to_pylist()
    plan = S.project(S.filter_(S.scan([STR, I32]), S.eq(R(s, "-", ""), S.lit("100200", STR))), [s, S.scalar_func("length", [R(s, ",", " , ")], I32)])
    got = _run(plan, t, 2)
    keep = [v for v in vals if _want("-", "", v) == "100200"]
    assert 0 < len(keep) < len(vals) and got.column(0).to_pylist() == keep and set(keep) == {"100-200"}
    assert got.column(1).to_pylist() == [len(_want(",", " , ", v)) for v in keep]
    lens = _run(S.project(S.scan([STR, I32]), [S.scalar_func("length", [R(s, r"[a-z]+", "${0}${0}")], I32)]), t, 1)
    assert lens.column(0).to_pylist() == [None if v is None else len(_want(r"[a-z]+", "${0}${0}", v)) for v in vals]


def test_one_long_row_among_short_ones(built):
    long = ("ab,12;" * 11_700)[:70_001]      # matches throughout; its neighbours' spans are four orders of magnitude shorter
    vals = ["a,b", long, None, "", "1,2;3", "x"] * 3 + ["é,é"]
    t = pa.table({"s": pa.array(vals, pa.utf8()), "k": pa.array(np.arange(len(vals), dtype=np.int32))})
    _check([("[,;]", " | "), ("[^0-9]", ""), (r"(\w+),(\d+)", "$2=$1"), ("", "-")], t)


def test_past_the_grids_first_step(built):
    """1 100 000 rows: beyond the 4096 x 256 rows at which the kernels' grid-stride loop takes a second step"""
    n = 1_100_000
    rng = np.random.default_rng(34)
    w = np.array(WORDS[:13], dtype=object)
    vals = w[rng.integers(0, 13, n)]
    t = pa.table({"s": pa.array(vals, pa.utf8(), mask=rng.random(n) < 0.1), "k": pa.array(np.arange(n, dtype=np.int32))})
    got = _run(S.project(S.scan([STR, I32]), [R(s, r"(\d+)-(\d+)", "$2/$1"), R(s, ",", "")]), t, 2)
    src = t.column(0).to_pylist()
    assert got.column(0).to_pylist() == [_want(r"(\d+)-(\d+)", "$2/$1", v) for v in src]
    assert got.column(1).to_pylist() == [_want(",", "", v) for v in src]


def test_what_regexp_replace_refuses(built):
    t = _table(10)
    for e, why in ((R(S.scalar_func("upper", [s], STR), "a", "b"), "Utf8 COLUMN"), (R(s, r"\p{L}", "x"), "not supported"), (R(s, "(a)", r"\1"), "backslash"),
                   (R(s, "(a)", "$2"), "Expects group index between 0 and 1, but got 2")):
        with pytest.raises(native.CometNativeException, match=why):
            _run(S.project(S.scan([STR, I32]), [e]), t, 1)


def test_a_result_beyond_2_gib_fails_the_task(built):
    """the empty pattern matches 2^20 + 1 times in a 1 MiB row: x 2100 bytes of replacement is 2.2 GB — found by the length pass, before anything is allocated"""
    t = pa.table({"s": pa.array(["short", "a" * (1 << 20)], pa.utf8()), "k": pa.array([0, 1], pa.int32())})
    with pytest.raises(native.CometNativeException, match="exceeds 2 GiB of string data"):
        _run(S.project(S.scan([STR, I32]), [R(s, "", "r" * 2100)]), t, 1)
