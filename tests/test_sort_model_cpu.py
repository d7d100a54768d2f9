"""tests/sort_model.py against the oracle's Sort (a stable Python comparison sort, oracle.py "sort"): the vectorised model the GPU sort tests compare the
device with is itself pinned here, on tables small enough for the comparison sort — every key type, ASC / DESC × NULLS FIRST / LAST, up to three keys,
fetch and skip.  The oracle is the authority: where they differ the model is wrong."""
import numpy as np
import pyarrow as pa
import pytest

from datafusion_comet_amd import serde as S

from tests import sort_model as M

CASES = M.key_cases(S, n=400, seed=7)
DIRS = [(False, False), (False, True), (True, False), (True, True)]      # (descending, nulls_last)


def _oracle(plan, table):
    from oracle import oracle as O
    return O.run_plan_to_arrow(S, plan, [table])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_one_key_and_behind_a_low_cardinality_key(built, case):
    t, f = case["table"], case["fields"]
    g, i = S.col(case["g"], S.T_INT32), S.col(case["id"], S.T_INT64)
    for desc, nl in DIRS:
        # alone (ties in row order: the oracle's sort is stable), and as second key behind g, whose direction is the opposite one
        for so, mo in (([(case["key"], desc, nl)], [(case["model"], desc, nl)]),
                       ([(g, not desc, not nl), (case["key"], desc, nl), (i, desc, nl)], [(case["g"], not desc, not nl), (case["model"], desc, nl), (case["id"], desc, nl)])):
            want = _oracle(S.sort(S.scan(f), so), t)
            M.assert_same_rows(want, t, M.expected_order(t, mo))


@pytest.mark.parametrize("fetch,skip", [(None, 0), (None, 5), (50, 0), (50, 7), (50, 50), (7, 50), (0, 0), (10_000, 3), (None, 10_000)])
def test_fetch_then_skip(built, fetch, skip):
    case = next(c for c in CASES if c["name"] == "float64")
    t, f = case["table"], case["fields"]
    so = [(S.col(case["g"], S.T_INT32), True, False), (case["key"], False, True)]
    mo = [(case["g"], True, False), (case["model"], False, True)]
    want = _oracle(S.sort(S.scan(f), so, fetch=fetch, skip=skip), t)
    M.assert_same_rows(want, t, M.expected_order(t, mo, fetch, skip))
    M.check_sorted(want, t, mo, fetch, skip, case["id"])


def test_three_keys_of_mixed_types(built):
    rng = np.random.default_rng(11)
    n = 2000
    d = next(c for c in M.key_cases(S, n=n, seed=3) if c["name"] == "decimal(38,10)")["table"].column(0)
    t = pa.table({"s": pa.array([None if rng.random() < 0.1 else "k%d" % int(x) for x in rng.integers(0, 4, n)], pa.string()),
                  "b": pa.array(rng.random(n) < 0.5, mask=rng.random(n) < 0.2), "d": d, "id": pa.array(np.arange(n, dtype=np.int64))})
    f = [S.T_STRING, S.T_BOOL, S.decimal(38, 10), S.T_INT64]
    for (d0, n0), (d1, n1), (d2, n2) in ((DIRS[0], DIRS[3], DIRS[1]), (DIRS[2], DIRS[1], DIRS[3]), (DIRS[3], DIRS[0], DIRS[2])):
        so = [(S.col(0, f[0]), d0, n0), (S.col(1, f[1]), d1, n1), (S.col(2, f[2]), d2, n2)]
        mo = [(0, d0, n0), (1, d1, n1), (2, d2, n2)]
        for fetch, skip in ((None, 0), (300, 11)):
            want = _oracle(S.sort(S.scan(f), so, fetch=fetch, skip=skip), t)
            M.assert_same_rows(want, t, M.expected_order(t, mo, fetch, skip))


def test_check_sorted_accepts_any_order_of_ties_and_nothing_else(built):
    """check_sorted on a result it must accept (tied rows shuffled, another choice of rows from the run a fetch cuts) and on results it must refuse"""
    rng = np.random.default_rng(5)
    n = 300
    t = pa.table({"k": pa.array(rng.integers(0, 3, n).astype(np.int32), mask=rng.random(n) < 0.1), "id": pa.array(np.arange(n, dtype=np.int64) * 3 + 1)})
    mo = [(0, False, False)]
    full = M.expected_order(t, mo)
    r = M.rank_keys(t, mo)
    model = full[:100]
    last = np.flatnonzero((r[full] == r[model[-1]]).all(axis=1))               # positions (in the full order) of the run the fetch cuts
    other = full.copy()
    other[last] = other[last][::-1]                                             # the same keys, other rows of the cut run in front
    for rows in (model, other[:100]):
        M.check_sorted(t.take(pa.array(rows)), t, mo, 100, 0, 1)
    M.check_sorted(t.take(pa.array(other[4:100])), t, mo, 100, 4, 1)
    inner = np.flatnonzero(~(r[model] == r[model[-1]]).all(axis=1))
    wrong_key = model.copy()
    wrong_key[0], wrong_key[-1] = model[-1], model[0]                           # keys out of order
    lost = model.copy()
    lost[inner[0]] = full[-1]                                                   # a row of another key smuggled in
    dup = model.copy()
    dup[inner[1]] = dup[inner[0]]                                               # a row twice
    for rows in (wrong_key, lost, dup, model[:99]):
        with pytest.raises(AssertionError):
            M.check_sorted(t.take(pa.array(rows)), t, mo, 100, 0, 1)
    # a row of a key that lies wholly inside the output replaced by … nothing of that key is left outside, so only a foreign id can stand in: refused
    forged = t.take(pa.array(model)).set_column(1, "id", pa.array(np.where(np.arange(100) == inner[0], 2, t.column(1).to_numpy()[model])))
    with pytest.raises(AssertionError):
        M.check_sorted(forged, t, mo, 100, 0, 1)
