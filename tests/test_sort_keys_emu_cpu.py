"""The key bytes generate_sort_keys writes, evaluated on the host (tests/emu run_sort_keys) and held against tests/sort_model.py — which
tests/test_sort_model_cpu.py pins to the oracle.  The executor's radix sort, its TopK select and Window's partition / peer flags all read nothing but these
bytes: per key type, ASC / DESC × NULLS FIRST / LAST, alone and as second key behind a low-cardinality Int32,
  1. rows ordered by their bytes (unsigned, lexicographic, the row index last) are in the model's order;
  2. two rows have equal bytes exactly when their keys are equal (NULL = NULL, −0.0 ≠ 0.0, NaNs by payload);
  3. a NULL key's value bytes are zero, its NULL byte is 0 under NULLS FIRST and 1 under NULLS LAST (a value's is the other one);
  4. the key is as wide as the header comment of generate_sort_keys promises: 1 + width per key, 16 value bytes for any decimal and for a computed string,
     the longest value + 4 for a Utf8 column."""
import os
import sys

import numpy as np
import pyarrow as pa
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from datafusion_comet_amd import native, serde as S  # noqa: E402
from tests import sort_model as M  # noqa: E402
from tests.emu import codegen_emu as E  # noqa: E402

CASES = M.key_cases(S, n=400, seed=7)
DIRS = [(False, False), (False, True), (True, False), (True, True)]      # (descending, nulls_last)


def _byte_order(K):
    return np.lexsort([np.arange(K.shape[0])] + [K[:, b] for b in range(K.shape[1] - 1, -1, -1)])


def _same_partition(a, b):
    """do the rows of two matrices fall into the same classes of equal rows?"""
    _, ia = np.unique(a, axis=0, return_inverse=True)
    _, ib = np.unique(b, axis=0, return_inverse=True)
    ia, ib = ia.reshape(-1), ib.reshape(-1)
    pairs = len(np.unique(np.stack([ia, ib], axis=1), axis=0))
    return pairs == ia.max() + 1 and pairs == ib.max() + 1


def _check(t, fields, so, mo, widths):
    K = E.run_sort_keys(S.sort(S.scan(fields), so), t)
    assert K.shape == (t.num_rows, sum(1 + w for w in widths)), (K.shape, widths)                                   # 4
    assert _byte_order(K).tolist() == M.expected_order(t, mo).tolist()                                              # 1
    r = M.rank_keys(t, mo)
    assert _same_partition(K, r)                                                                                    # 2
    at = 0
    for k, ((_, _, nulls_last), w) in enumerate(zip(mo, widths)):                                                   # 3
        null = r[:, 2 * k] == (1 if nulls_last else 0)
        assert (K[null, at] == (1 if nulls_last else 0)).all() and (K[~null, at] == (0 if nulls_last else 1)).all()
        assert not K[null, at + 1:at + 1 + w].any(), "a NULL key carries value bytes"
        # … and within ONE key, equal bytes ⇔ equal key: what Window compares per partition / order key
        assert _same_partition(K[:, at:at + 1 + w], r[:, 2 * k:2 * k + 2])
        at += 1 + w


def _width(case):
    if case["width"] is not None:
        return case["width"]
    return max(len(v.encode()) for v in case["table"].column(0).to_pylist() if v is not None) + 4


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_key_bytes_order_and_equality(built, case):
    t, f = case["table"], case["fields"]
    assert t.column(0).null_count > 0
    g = S.col(case["g"], S.T_INT32)
    w = _width(case)
    for desc, nl in DIRS:
        _check(t, f, [(case["key"], desc, nl)], [(case["model"], desc, nl)], [w])
        _check(t, f, [(g, not desc, nl), (case["key"], desc, nl)], [(case["g"], not desc, nl), (case["model"], desc, nl)], [4, w])


def test_key_without_nulls_and_of_a_sliced_column(built):
    """a column that arrives without a validity bitmap (the generated code reads none), and a Utf8 column whose Arrow offset is not zero"""
    for name in ("int16", "float32", "decimal(9,2)", "utf8"):
        case = next(c for c in CASES if c["name"] == name)
        t = case["table"]
        t = t.set_column(0, "c0", t.column(0).combine_chunks().fill_null(t.column(0).drop_null()[0]))
        _check(t, case["fields"], [(case["key"], True, False)], [(0, True, False)], [_width(case)])
    case = next(c for c in CASES if c["name"] == "utf8")
    t = case["table"].slice(37, 200).combine_chunks()
    assert t.column(0).chunk(0).offset == 37
    w = max(len(v.encode()) for v in t.column(0).to_pylist() if v is not None) + 4
    _check(t, case["fields"], [(case["key"], False, True)], [(0, False, True)], [w])


def test_key_layout_of_six_utf8_columns_and_the_seventh_refused(built):
    rng = np.random.default_rng(2)
    n = 200
    words = ["", "a", "ab", "b", "long-%s" % ("x" * 40)]
    cols = [pa.array([None if rng.random() < 0.1 else words[int(x)][:3 + 10 * c] for x in rng.integers(0, len(words), n)], pa.string()) for c in range(7)]
    t = pa.table(cols, names=["s%d" % c for c in range(7)])
    f = [S.T_STRING] * 7
    so = [(S.col(c, S.T_STRING), bool(c & 1), bool(c & 2)) for c in range(6)]
    widths = [max(len(v) for v in cols[c].to_pylist() if v is not None) + 4 for c in range(6)]
    _check(t, f, so, [(c, bool(c & 1), bool(c & 2)) for c in range(6)], widths)
    d = native.plan_codegen(S.sort(S.scan(f), so).encode(), [True] * 7)
    assert d["sort_key_bytes"] == 6 and d["sort_str_cols"] == [0, 1, 2, 3, 4, 5] and d["kernels"] == ["k_sortkey"]      # the fixed part: six NULL bytes
    with pytest.raises(native.CometNativeException, match="more than 6 Utf8 sort keys"):
        native.plan_codegen(S.sort(S.scan(f), so + [(S.col(6, S.T_STRING), False, False)]).encode(), [True] * 7)
    with pytest.raises(native.CometNativeException, match="directly over its Scan"):
        native.plan_codegen(S.sort(S.filter_(S.scan(f), S.is_not_null(S.col(0, S.T_STRING))), so).encode(), [True] * 7)


def test_fixed_key_wider_than_255_bytes_is_refused(built):
    f = [S.decimal(38, 10)] * 16
    so = [(S.col(c, f[c]), False, False) for c in range(16)]      # 16 × 17 = 272 bytes
    with pytest.raises(native.CometNativeException, match="wider than 255 bytes"):
        native.plan_codegen(S.sort(S.scan(f), so).encode(), [False] * 16)
    d = native.plan_codegen(S.sort(S.scan(f[:15]), so[:15]).encode(), [False] * 15)
    assert d["sort_key_bytes"] == 255
