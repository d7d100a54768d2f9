"""oracle/oracle.py against the per-row model (tests/dead_rows_model.py) on the plans of tests/test_dead_rows_gpu.py: value, NULL-ness and error class.  The
oracle is what every other GPU test compares with; it used to evaluate every branch of a conditional over all rows, so an error in a branch no row reaches
was raised by the oracle as well, and "GPU == oracle" held.  This module keeps it lazy.  The oracle walks columns, not tiles: it gets the dead offenders, the
rows around them and a prefix of the table rather than all 20 003 rows.

Also here: the generated source of join plans WITHOUT a raise site, against the SHA-256 recorded from the commit before the guard
(tests/golden/dead_rows_join_codegen.json) — the tuned probe paths are what they were."""
import hashlib
import json
import os

import numpy as np
import pyarrow as pa
import pytest

from datafusion_comet_amd import native, serde as S, tpch
from oracle import oracle as O
from tests import dead_rows_model as M
from tests import test_dead_rows_gpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOME = np.array(sorted(set(range(1500)) | {r + d for r in G.DEAD for d in (-1, 0, 1) if 0 <= r + d < G.N}))


def _some(data):
    """→ the table and the model's rows of the sample"""
    rows = data.rows()
    return data.table().take(pa.array(SOME)), [rows[i] for i in SOME]


def _oracle_raises(plan, table, site):
    with pytest.raises(O.OracleError) as ei:
        O.run_plan_to_arrow(S, plan, table)
    assert str(ei.value).split()[0] == site.cls.split(".")[0], (site.name, ei.value)


def test_null_operands():
    plan, types, data = G.null_operand_case()
    table, rows = _some(data)
    G.check_equal(O.run_plan_to_arrow(S, plan, table), types, M.run([s.expr for s in G.SITES], rows))
    for k, s in enumerate(G.SITES):
        live = G.offend_live(data.copy(), G.DEAD[k], s)
        _oracle_raises(plan, _some(live)[0], s)


@pytest.mark.parametrize("form", list(G.FORMS))
def test_unpicked_branches(form):
    plan, types, cols, data, live_g = G.branch_case(form)
    table, rows = _some(data)
    G.check_eager_raises(cols, rows)
    G.check_equal(O.run_plan_to_arrow(S, plan, table), types, M.run([e for _, e in cols], rows))
    for k, s in enumerate(G.SITES):
        live = G.offend_live(data.copy(), G.DEAD[k], s, g=live_g)
        _oracle_raises(plan, _some(live)[0], s)


@pytest.mark.parametrize("name", ["filter_project", "filter_filter", "filter_aggregate", "filter_isnotnull_project"])
def test_rows_a_lower_filter_drops(name):
    plan, types, preds, exprs, dead = G.filter_cases()[name]
    data = G.filter_data(name)
    table, rows = _some(data)
    got = O.run_plan_to_arrow(S, plan, table)
    G.check_equal(G._sorted_by_key(got) if exprs is None else got, types, G.filter_want(name, rows))
    for k, s in enumerate(G.B_SITES):
        live = G.offend_live(data.copy(), G.DEAD[k + 2], s, g=1)
        _oracle_raises(plan, _some(live)[0], s)


def test_one_expression_under_two_guards():
    for s in (G.SITE["idiv0"], G.SITE["add"]):
        exprs = [G._guarded(s, "g"), G._guarded(s, "h")]
        plan = S.project(S.scan(G.FIELDS), exprs)
        data = G.offend_all(G.base(), G.DEAD, sites=[s], g=0, h=2)
        table, rows = _some(data)
        G.check_equal(O.run_plan_to_arrow(S, plan, table), [s.T, s.T], M.run(exprs, rows))
        for guards in (dict(g=1, h=0), dict(g=0, h=1)):
            _oracle_raises(plan, _some(G.offend_live(data.copy(), G.DEAD[4], s, **guards))[0], s)


def test_parent_of_a_guarded_expression_used_bare():
    for s in (G.SITE["idiv0"], G.SITE["add"]):
        exprs = G.parent_used_bare_exprs(s)
        plan = S.project(S.scan(G.FIELDS), exprs)
        data = G.base()
        table, rows = _some(data)
        G.check_equal(O.run_plan_to_arrow(S, plan, table), [G.BOOL, G.BOOL], M.run(exprs, rows))
        for g in (0, 1):
            _oracle_raises(plan, _some(G.offend_live(data.copy(), G.DEAD[4], s, g=g))[0], s)


def test_the_model_tells_lazy_from_eager():
    """the model itself: a guarded division by zero raises eagerly and not lazily; a NULL operand never raises"""
    e = S.if_(S.eq(G.C["g"], S.lit(1, G.I32)), G.SITE["idiv0"].expr, S.lit(None, G.I64))
    row = list(G.base().rows()[0])
    row[G.NAMES.index("g")], row[G.NAMES.index("p")], row[G.NAMES.index("q")] = 0, 5, 0
    assert M.error_of([e], [tuple(row)]) is None and M.error_of([e], [tuple(row)], eager=True).error_class == "DIVIDE_BY_ZERO"
    row[G.NAMES.index("q")] = None
    assert M.error_of([e], [tuple(row)], eager=True) is None
    row[G.NAMES.index("g")], row[G.NAMES.index("q")] = 1, 0
    assert M.error_of([e], [tuple(row)]).error_class == "DIVIDE_BY_ZERO"


def test_joins_without_a_raise_site_generate_the_source_they_did():
    with open(os.path.join(ROOT, "tests", "golden", "dead_rows_join_codegen.json")) as f:
        want = json.load(f)
    got = join_codegen_plans()
    assert sorted(got) == sorted(want)
    for name, (plan, hv) in got.items():
        src = native.plan_codegen(plan.encode(), hv)["source"].encode()
        assert (hashlib.sha256(src).hexdigest(), len(src)) == (want[name]["sha256"], want[name]["bytes"]), name


def join_codegen_plans():
    """name → (plan, has_valid per input column): TPC-H Q3's joins and tests/test_join_paths_gpu.py's join with and without a residual condition"""
    from tests.test_hash_join_gpu import CFIELDS
    from tests.test_join_paths_gpu import _join
    cond = S.gt(S.col(1, S.T_INT32), S.col(4, S.T_INT32))
    ncols = 2 * len(CFIELDS)
    plans = {"paths_join": (_join(), [True, False, False] * 2), "paths_join_no_nulls": (_join(), [False] * ncols),
             "paths_join_residual": (_join(cond=cond), [True, False, False] * 2), "paths_semi_residual": (_join(S.LEFT_SEMI, cond=cond), [True, False, False] * 2)}
    # Q3 = aggregate ← project ← join 2 (project ← join 1 (customer chain, orders chain), lineitem chain): each join with its fused chains; join 2's left
    # side, join 1's output, as a Scan
    j2 = tpch.q3_plan().children[0].children[0]
    j1 = j2.children[0].children[0]
    j2 = S.hash_join(S.scan([S.T_INT64, S.T_DATE, S.T_INT32]), j2.children[1], j2.left_keys, j2.right_keys, S.INNER, S.BUILD_LEFT)
    for name, plan, ncols in (("q3_join1", j1, 6), ("q3_join2", j2, 7)):
        plans[name] = (plan, [False] * ncols)
        plans[name + "_nullable"] = (plan, [True] * ncols)
    return plans
