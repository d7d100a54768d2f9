"""ANSI errors are raised only for the rows Spark evaluates.  Every case has two sides: (1) rows that WOULD raise sit where the engine must not evaluate them
— under a NULL operand, below a Filter that drops them, in a branch of If / CaseWhen / coalesce the row does not pick, on a join's dropped rows and unmatched
pairs — and the query succeeds with exactly the values of the per-row model (tests/dead_rows_model.py: Python ints, lazy); (2) the same data with ONE live
offender raises CometQueryExecutionException with the site's error class and, where the error names a value, that row's value (the dead offenders hold others).
Side 1 is never vacuous: the dead offenders are counted, and the model run with eager=True — every child of a conditional first — raises the site's class
over the same rows (for rows under a NULL or below a Filter: over the offenders made live).

Raise sites (one per error kind reachable through serde.py): Int64 add, Int32 subtract, Int64 multiply overflow; Long.MinValue div -1; Int64 `div` by zero
(DIVIDE_BY_ZERO); Int64 remainder by zero; Decimal divide by zero; wide Decimal multiply overflow (bit 0); Int64 → Int32 and Float64 → Int64 cast overflow;
CheckOverflow with fail_on_error; Int64 → Decimal(3,2) beyond the precision; a malformed string → Int32; abs and unary minus of the minimum.
Left out: the string → date / timestamp / decimal casts (the same raise_with_string statement as string → Int32), Decimal → Int32 and Float → Decimal casts
(the same raise_value call as the two numeric casts here), decimal remainder and float remainder by zero (the Int64 remainder's raise_if), element_at's index
errors (lists: another input shape), round()'s and the timestamp casts' overflow bits (18, 11, 12: refusals of this engine, not Spark errors), and the
aggregates' overflow flags (raised by the sink's emit, not by a row's expression).

Pipelines run 20 003 rows; dead offenders sit at rows 0, 255, 256, the last row of a tile and the first of the next (4095 / 4096, 8191 / 8192), n - 1 and
forty rows between; the live offender of each site takes one of these in turn.  The non-join tests run on the host too (tests/test_codegen_emu_cpu.py)."""
import json
from decimal import Decimal

import numpy as np
import pyarrow as pa
import pytest

from datafusion_comet_amd import native, serde as S
from tests import dead_rows_model as M

pytestmark = pytest.mark.gpu

I32, I64, F64, STR, BOOL = S.T_INT32, S.T_INT64, S.T_DOUBLE, S.T_STRING, S.T_BOOL
D12, D38 = S.decimal(12, 2), S.decimal(38, 0)
MIN32, MIN64, MAX64 = -(1 << 31), -(1 << 63), (1 << 63) - 1
N = 20_003

COLS = [("g", I32), ("h", I32), ("x", I64), ("u", I32), ("i", I64), ("p", I64), ("q", I64), ("p2", I64), ("r", I64), ("t", I64), ("d", D12), ("e", D12), ("w", D38),
        ("a", I64), ("f", F64), ("c", D12), ("b", I64), ("s", STR), ("m", I32), ("n", I64)]
NAMES = [c for c, _ in COLS]
FIELDS = [t for _, t in COLS]
C = {name: S.col(k, t) for k, (name, t) in enumerate(COLS)}


class Site:
    """one raise site: its expression, result type, Spark error class, the operand values that make row k offend (distinct per k where the error names the
    value), the operand to put NULL in case (a) (by k, in turn), and how the error's JSON spells the offending value"""

    def __init__(self, name, expr, T, cls, offend, nulls, spelled=None):
        self.name, self.expr, self.T, self.cls, self.offend, self.nulls, self.spelled = name, expr, T, cls, offend, nulls, spelled


def _idiv(a, b):
    return S.integral_divide(a, I64, b, I64, S.ANSI, check_divide_overflow=True)


def _neg(a):
    return S.Expr("unary_minus", [a], fail_on_error=True)


SITES = [
    Site("add", S.math("add", C["x"], S.lit(5, I64), I64, S.ANSI), I64, "ARITHMETIC_OVERFLOW", lambda k: {"x": MAX64 - k % 5}, ["x"]),
    Site("sub", S.math("subtract", C["u"], S.lit(7, I32), I32, S.ANSI), I32, "ARITHMETIC_OVERFLOW", lambda k: {"u": MIN32 + k % 7}, ["u"]),
    Site("mul", S.math("multiply", C["i"], S.lit(4096, I64), I64, S.ANSI), I64, "ARITHMETIC_OVERFLOW", lambda k: {"i": (1 << 52) + k}, ["i"]),
    Site("idiv0", _idiv(C["p"], C["q"]), I64, "DIVIDE_BY_ZERO", lambda k: {"p": 100 + k, "q": 0}, ["q", "p"]),
    Site("idivmin", _idiv(C["p2"], S.lit(-1, I64)), I64, "ARITHMETIC_OVERFLOW", lambda k: {"p2": MIN64}, ["p2"]),
    Site("rem", S.math("remainder", C["r"], C["t"], I64, S.ANSI), I64, "REMAINDER_BY_ZERO", lambda k: {"r": 7 + k, "t": 0}, ["t", "r"]),
    Site("ddiv", S.math("divide", C["d"], C["e"], S.decimal(27, 15), S.ANSI), S.decimal(27, 15), "DIVIDE_BY_ZERO", lambda k: {"d": 1000 + k, "e": 0}, ["e", "d"]),
    Site("dmul", S.math("multiply", C["w"], S.lit(10 ** 19, D38), D38, S.ANSI), D38, "ARITHMETIC_OVERFLOW", lambda k: {"w": 10 ** 20 + k}, ["w"]),
    Site("casti", S.cast(C["a"], I32, S.ANSI), I32, "CAST_OVERFLOW", lambda k: {"a": (1 << 31) + k}, ["a"], lambda v: "%dL" % v["a"]),
    Site("castf", S.cast(C["f"], I64, S.ANSI), I64, "CAST_OVERFLOW", lambda k: {"f": (k % 8 + 1) * 1e19 if k < 1000 else 9e19}, ["f"], lambda v: "%dE19D" % round(v["f"] / 1e19)),      # (Rust's {:E} of the double, as the reference spells it)
    Site("chkov", S.check_overflow(S.math("multiply", C["c"], C["c"], S.decimal(25, 4)), S.decimal(20, 4), True), S.decimal(20, 4), "NUMERIC_VALUE_OUT_OF_RANGE.WITH_SUGGESTION",
         lambda k: {"c": 10 ** 11 + k}, ["c"], lambda v: str(v["c"] ** 2)),
    Site("castdec", S.cast(C["b"], S.decimal(3, 2), S.ANSI), S.decimal(3, 2), "NUMERIC_VALUE_OUT_OF_RANGE.WITH_SUGGESTION", lambda k: {"b": 1000 + k}, ["b"], lambda v: str(v["b"])),
    Site("caststr", S.cast(C["s"], I32, S.ANSI), I32, "CAST_INVALID_INPUT", lambda k: {"s": "%dx" % k}, ["s"], lambda v: v["s"]),
    Site("abs", S.scalar_func("abs", [C["m"], S.lit(True, BOOL)], I32), I32, "ARITHMETIC_OVERFLOW", lambda k: {"m": MIN32}, ["m"]),
    Site("neg", _neg(C["n"]), I64, "ARITHMETIC_OVERFLOW", lambda k: {"n": MIN64}, ["n"]),
]
SITE = {s.name: s for s in SITES}
LIVE_K = 5000      # the live offender's k: its value differs from every dead offender's (k < 100)

POS = [0, 255, 256, 4095, 4096, 8191, 8192, N - 1]
DEAD = sorted(set(POS) | set(range(300, N, 493)))      # 8 + 40 rows


# ----------------------------------------------------------------------------------------------- data


class Data:
    """columns as Python lists (a decimal is its unscaled integer) with a NULL mask each; the Arrow arrays keep a NULL slot's value in the data buffer"""

    def __init__(self, vals, null):
        self.vals, self.null, self._arrow = vals, null, {}

    def copy(self):
        d = Data({k: list(v) for k, v in self.vals.items()}, {k: v.copy() for k, v in self.null.items()})
        d._arrow = dict(self._arrow)
        return d

    def set(self, row, null=(), **kv):
        """values into a row; the columns of `null` become NULL there, the others that are set become valid"""
        for name, v in kv.items():
            self.vals[name][row] = v
            self.null[name][row] = name in null
            self._arrow.pop(name, None)
        return self

    def column(self, name):
        if name not in self._arrow:
            self._arrow[name] = _arrow_array(dict(COLS)[name], self.vals[name], self.null[name])
        return self._arrow[name]

    def table(self, names=NAMES):
        return pa.table([self.column(n) for n in names], names=list(names))

    def rows(self, names=NAMES):
        return list(zip(*[[None if z else v for v, z in zip(self.vals[n], self.null[n])] for n in names]))


def _arrow_array(t, vals, null):
    n = len(vals)
    vb = pa.py_buffer(np.packbits(~null, bitorder="little").tobytes()) if null.any() else None
    nulls = int(null.sum())
    if t.type_id == S.DECIMAL:
        return pa.Array.from_buffers(pa.decimal128(t.precision, t.scale), n, [vb, pa.py_buffer(b"".join(int(v).to_bytes(16, "little", signed=True) for v in vals))], null_count=nulls)
    if t.type_id == S.STRING:
        raw = [v.encode() for v in vals]
        offs = np.zeros(n + 1, np.int32)
        offs[1:] = np.cumsum([len(b) for b in raw])
        return pa.Array.from_buffers(pa.utf8(), n, [vb, pa.py_buffer(offs.tobytes()), pa.py_buffer(b"".join(raw))], null_count=nulls)
    np_t = {S.INT32: np.int32, S.INT64: np.int64, S.DOUBLE: np.float64}[t.type_id]
    return pa.array(np.array(vals, dtype=np_t), mask=null if null.any() else None)


def physical(arr, row):
    """what the Arrow array's data buffer holds at `row`, valid or not"""
    if isinstance(arr, pa.ChunkedArray):
        arr = arr.combine_chunks()
    bufs, row = arr.buffers(), row + arr.offset
    if pa.types.is_string(arr.type):
        o = np.frombuffer(bufs[1], np.int32)
        return bufs[2].to_pybytes()[o[row]:o[row + 1]].decode()
    if pa.types.is_decimal(arr.type):
        return int.from_bytes(bufs[1].to_pybytes()[16 * row:16 * row + 16], "little", signed=True)
    return np.frombuffer(bufs[1], arr.type.to_pandas_dtype())[row].item()


def _boring(n, seed):
    """rows no site raises for; every column but the guards holds some NULLs (so that every variant of the data generates the same code)"""
    rng = np.random.default_rng(seed)
    ints = lambda lo, hi: [int(v) for v in rng.integers(lo, hi, n)]
    nonzero = lambda hi: [int(v) for v in rng.integers(1, hi, n) * rng.choice([-1, 1], n)]
    vals = {"g": ints(0, 3), "h": ints(0, 3), "x": ints(-10 ** 6, 10 ** 6), "u": ints(-1000, 1000), "i": ints(-10 ** 6, 10 ** 6), "p": ints(-10 ** 6, 10 ** 6), "q": nonzero(1000),
            "p2": ints(-10 ** 6, 10 ** 6), "r": ints(-10 ** 6, 10 ** 6), "t": nonzero(1000), "d": ints(-10 ** 9, 10 ** 9), "e": nonzero(10 ** 6), "w": ints(-10 ** 9, 10 ** 9),
            "a": ints(-10 ** 6, 10 ** 6), "f": [float(v) for v in rng.integers(-10 ** 6, 10 ** 6, n) / 8], "c": ints(-10 ** 8, 10 ** 8), "b": ints(-9, 10),
            "s": [str(v) for v in rng.integers(-10 ** 5, 10 ** 5, n)], "m": ints(-1000, 1000), "n": ints(-10 ** 6, 10 ** 6)}
    null = {name: (rng.random(n) < 0.03) if name not in ("g", "h") else np.zeros(n, bool) for name in NAMES}
    for name in NAMES[2:]:
        null[name][DEAD] = False
        null[name][1] = True      # (row 1 is nobody's: at least one NULL per column whatever the variant sets)
    return Data(vals, null)


_BASE = {}


def base(n=N, seed=1):
    if (n, seed) not in _BASE:
        _BASE[n, seed] = _boring(n, seed)
    return _BASE[n, seed].copy()


def offend_all(data, rows, sites=SITES, null_operand=False, **guards):
    """every site offends in every row of `rows` (k = the row's rank), the guards set as given (a tuple: its values in turn); null_operand: one operand of
    each site is NULL there"""
    for k, row in enumerate(rows):
        for s in sites:
            data.set(row, null=[s.nulls[k % len(s.nulls)]] if null_operand else (), **s.offend(k))
        data.set(row, **{name: v[k % len(v)] if isinstance(v, tuple) else v for name, v in guards.items()})
    return data


def offend_live(data, row, site, **guards):
    """row `row` becomes an ordinary valid row but for `site`, which offends with the live value"""
    b = base(len(data.vals["g"]))
    data.set(row, **{name: b.vals[name][row] for name in NAMES})
    return data.set(row, **site.offend(LIVE_K), **guards)


# ----------------------------------------------------------------------------------------------- running and comparing


def _run(plan, table, ncols):
    out = native.execute_to_table([native.HostInput.from_table(table)], ncols, plan.encode())
    return pa.Table.from_batches(out) if out else None


def _spelled(T, v):
    """a model value as pyarrow's to_pylist() gives it"""
    if v is None or T.type_id != S.DECIMAL:
        return v
    return Decimal(v).scaleb(-T.scale)


def check_equal(got, types, want_cols):
    """every output column equals the model's, value and NULL-ness, exactly"""
    nrows = len(want_cols[0]) if want_cols else 0
    assert (got.num_rows if got is not None else 0) == nrows
    if nrows == 0:
        return
    assert got.num_columns == len(want_cols)
    for k, (T, want) in enumerate(zip(types, want_cols)):
        g = got.column(k).to_pylist()
        w = [_spelled(T, v) for v in want]
        if g != w:
            bad = next(r for r in range(nrows) if g[r] != w[r])
            raise AssertionError(f"column {k}, row {bad}: got {g[bad]!r}, the model has {w[bad]!r}")


def check_raises(run, site, live_values=None):
    """the run fails with the site's error class — and the live row's value where the error's JSON names one"""
    with pytest.raises(native.CometQueryExecutionException) as ei:
        run()
    j = json.loads(str(ei.value))
    assert j["errorClass"] == site.cls, (site.name, j)
    if site.spelled is not None:
        assert j["params"]["value"] == site.spelled(live_values if live_values is not None else site.offend(LIVE_K)), (site.name, j)


def check_eager_raises(exprs_by_site, rows):
    """the case is not vacuous: evaluated eagerly, every site's expression raises its class over these rows"""
    for site, ex in exprs_by_site:
        err = M.error_of([ex], rows, eager=True)
        assert err is not None and err.error_class == site.cls, (site.name, err)


def count_offenders(site, rows):
    """the rows whose operands, were they evaluated, make the site raise"""
    f = M.compile_expr(site.expr)
    n = 0
    for row in rows:
        try:
            f(row)
        except M.SparkError:
            n += 1
    return n


# ----------------------------------------------------------------------------------------------- (a) NULL operands


def null_operand_case():
    """→ plan, result types, side-1 data"""
    plan = S.project(S.scan(FIELDS), [s.expr for s in SITES])
    return plan, [s.T for s in SITES], offend_all(base(), DEAD, null_operand=True)


def test_a_null_operand_raises_nothing(built):
    plan, types, data = null_operand_case()
    table = data.table()
    for k, row in enumerate(DEAD):
        for s in SITES:      # the slot under the cleared validity bit physically holds the offending value
            name = s.nulls[k % len(s.nulls)]
            col = table.column(name)
            assert not col[row].is_valid and physical(col, row) == s.offend(k)[name], (s.name, row)
    valid_again = offend_all(base(), DEAD).rows()
    for s in SITES:
        assert count_offenders(s, valid_again) == len(DEAD) > 0
    check_eager_raises([(s, s.expr) for s in SITES], valid_again)      # (with the operands valid, every site raises)
    check_equal(_run(plan, table, len(SITES)), types, M.run([s.expr for s in SITES], data.rows()))
    for k, s in enumerate(SITES):
        row = DEAD[(k * 7) % len(DEAD)] if k >= len(POS) else POS[k]
        live = offend_live(data.copy(), row, s)
        assert M.error_of([x.expr for x in SITES], live.rows()[row:row + 1]).error_class == s.cls
        check_raises(lambda: _run(plan, live.table(), len(SITES)), s)


# ----------------------------------------------------------------------------------------------- (c) unpicked branches


def _lit(T, v=7):
    return S.lit(v, T)


def _g(v):
    return S.eq(C["g"], S.lit(v, I32))


def _nullable(T):
    """NULL where g = 1, else 7"""
    return S.if_(_g(1), S.lit(None, T), _lit(T))


# form → (expression of a site, the guard values under which the site is NOT evaluated, the guard value under which it is)
FORMS = {
    "if_then": (lambda s: S.if_(_g(1), s.expr, S.lit(None, s.T)), (0, 2), 1),
    "if_else": (lambda s: S.if_(_g(1), _lit(s.T), s.expr), (1,), 0),
    "case_then": (lambda s: S.case_when([(_g(1), s.expr)]), (0, 2), 1),
    "case_then_with_else": (lambda s: S.case_when([(_g(1), s.expr)], _lit(s.T)), (0, 2), 1),
    "case_later_when": (lambda s: S.case_when([(_g(0), _lit(s.T)), (S.gt(s.expr, _lit(s.T)), _lit(s.T, 8))], _lit(s.T, 9)), (0,), 2),
    "case_else": (lambda s: S.case_when([(_g(0), _lit(s.T))], s.expr), (0,), 1),
    "coalesce_as_case": (lambda s: S.case_when([(S.is_not_null(_nullable(s.T)), _nullable(s.T))], s.expr), (0, 2), 1),
    "coalesce_function": (lambda s: S.scalar_func("coalesce", [_nullable(s.T), s.expr], s.T), (0, 2), 1),
    "if_inside_case_then": (lambda s: S.case_when([(S.gt_eq(C["g"], S.lit(1, I32)), S.if_(_g(1), s.expr, _lit(s.T)))]), (0, 2), 1),
}
# behind an argument that is never NULL nothing is evaluated, whatever the row: extra columns of the two coalesce plans
NEVER = {"coalesce_as_case": lambda s: S.case_when([(S.is_not_null(_lit(s.T)), _lit(s.T))], s.expr),
         "coalesce_function": lambda s: S.scalar_func("coalesce", [_lit(s.T), s.expr], s.T)}


def branch_case(form):
    """→ plan, result types, [(site, its expression)], side-1 data, the guard value that makes a row live"""
    make, dead_g, live_g = FORMS[form]
    cols = [(s, make(s)) for s in SITES]
    if form in NEVER:      # (a pipeline has 22 output columns at the most: six sites, one per error class)
        cols += [(SITE[name], NEVER[form](SITE[name])) for name in ("add", "idiv0", "rem", "casti", "chkov", "caststr")]
    data = offend_all(base(), DEAD, g=dead_g)
    return S.project(S.scan(FIELDS), [e for _, e in cols]), [s.T for s, _ in cols], cols, data, live_g


@pytest.mark.parametrize("form", list(FORMS))
def test_c_unpicked_branch_raises_nothing(built, form):
    plan, types, cols, data, live_g = branch_case(form)
    rows = data.rows()
    for s in SITES:
        assert count_offenders(s, rows) == len(DEAD) > 0
    check_eager_raises(cols, rows)
    check_equal(_run(plan, data.table(), len(cols)), types, M.run([e for _, e in cols], rows))
    for k, s in enumerate(SITES):
        row = DEAD[(k * 7) % len(DEAD)] if k >= len(POS) else POS[k]
        live = offend_live(data.copy(), row, s, g=live_g)
        assert M.error_of([e for _, e in cols], live.rows()[row:row + 1]).error_class == s.cls
        check_raises(lambda: _run(plan, live.table(), len(cols)), s)


def _guarded(s, col="g"):
    return S.if_(S.eq(C[col], S.lit(1, I32)), s.expr, S.lit(None, s.T))


@pytest.mark.parametrize("guarded_first", [False, True])
def test_c_one_expression_guarded_and_unguarded_raises_for_the_unguarded_use(built, guarded_first):
    """the common-subexpression memo must not hand the guarded lowering's raise to the unguarded use (nor the reverse): x div y once bare and once under
    If(g = 1) raises for an offender whose g is 0"""
    for s in (SITE["idiv0"], SITE["add"]):
        exprs = [_guarded(s), s.expr] if guarded_first else [s.expr, _guarded(s)]
        plan = S.project(S.scan(FIELDS), exprs)
        data = base()
        check_equal(_run(plan, data.table(), 2), [s.T, s.T], M.run(exprs, data.rows()))
        for row in (POS[3], N - 1):
            live = offend_live(data.copy(), row, s, g=0)
            assert M.error_of(exprs, live.rows()[row:row + 1]).error_class == s.cls
            check_raises(lambda: _run(plan, live.table(), 2), s)


def parent_used_bare_exprs(s):
    """x div y twice inside one branch — the second use takes the branch's lowering from the memo — and the non-raising parent of that second use, x div y < 9,
    once more outside every branch"""
    lo, hi = S.lit(3, s.T), S.lit(9, s.T)
    return [S.if_(_g(1), S.and_(S.gt(s.expr, lo), S.lt(s.expr, hi)), S.lit(None, BOOL)), S.lt(s.expr, hi)]


def test_c_parent_of_a_guarded_expression_used_bare_raises(built):
    """the memo must not hand out what was lowered AROUND a guarded raising expression either: the bare x div y < 9 raises for an offender whose g is 0"""
    for s in (SITE["idiv0"], SITE["add"]):
        exprs = parent_used_bare_exprs(s)
        plan = S.project(S.scan(FIELDS), exprs)
        data = base()
        check_equal(_run(plan, data.table(), 2), [BOOL, BOOL], M.run(exprs, data.rows()))
        for row, g in ((POS[2], 0), (N - 1, 2), (POS[5], 1)):
            live = offend_live(data.copy(), row, s, g=g)
            assert M.error_of(exprs, live.rows()[row:row + 1]).error_class == s.cls
            check_raises(lambda: _run(plan, live.table(), 2), s)


def test_c_one_expression_under_two_guards(built):
    """x div y under If(g = 1) and under If(h = 1): an offender raises when either guard picks it, and only then"""
    for s in (SITE["idiv0"], SITE["add"]):
        exprs = [_guarded(s, "g"), _guarded(s, "h")]
        plan = S.project(S.scan(FIELDS), exprs)
        data = offend_all(base(), DEAD, sites=[s], g=0, h=2)
        rows = data.rows()
        assert count_offenders(s, rows) == len(DEAD) > 0
        check_eager_raises([(s, e) for e in exprs], rows)
        check_equal(_run(plan, data.table(), 2), [s.T, s.T], M.run(exprs, rows))
        for row, guards in ((POS[1], dict(g=1, h=0)), (POS[4], dict(g=0, h=1))):
            live = offend_live(data.copy(), row, s, **guards)
            assert M.error_of(exprs, live.rows()[row:row + 1]).error_class == s.cls
            check_raises(lambda: _run(plan, live.table(), 2), s)


# ----------------------------------------------------------------------------------------------- (b) rows a Filter lower in the chain drops

B_SITES = [SITE["idiv0"], SITE["add"]]


def _kept(preds, rows):
    """the rows every predicate — evaluated bottom-up, the next one only where the one below it kept the row — is TRUE for"""
    fs = [M.compile_expr(p) for p in preds]
    return [row for row in rows if all(f(row) is True for f in fs)]


def filter_cases():
    """name → (plan, result types, predicates bottom-up, projected expressions | None for the aggregate, dead-row settings)"""
    scan = S.scan(FIELDS)
    exprs = [s.expr for s in B_SITES]
    keep = _g(1)
    up = [S.gt(SITE["idiv0"].expr, S.lit(-10 ** 7, I64)), S.gt(SITE["add"].expr, S.lit(-10 ** 8, I64))]
    agg = S.hash_agg(S.filter_(scan, keep), [SITE["add"].expr], [S.sum_(SITE["idiv0"].expr, I64)])
    return {"filter_project": (S.project(S.filter_(scan, keep), exprs), [I64, I64], [keep], exprs, dict(g=0)),
            "filter_filter": (S.project(S.filter_(S.filter_(S.filter_(scan, keep), up[0]), up[1]), [C["x"], C["p"]]), [I64, I64], [keep] + up, [C["x"], C["p"]], dict(g=2)),
            "filter_aggregate": (agg, [I64, I64], [keep], None, dict(g=0)),
            "filter_isnotnull_project": (S.project(S.filter_(scan, S.is_not_null(C["q"])), exprs), [I64, I64], [S.is_not_null(C["q"])], exprs, dict(null=["q"]))}


def filter_data(name):
    dead = filter_cases()[name][4]
    data = offend_all(base(), DEAD, sites=B_SITES, **{k: v for k, v in dead.items() if k != "null"})
    for row in DEAD if "null" in dead else ():
        data.set(row, null=dead["null"], q=0)
    return data


def filter_want(name, rows):
    """the model's output columns for the plan `name` over `rows` (the aggregate's: sorted by key)"""
    _, _, preds, exprs, _ = filter_cases()[name]
    kept = _kept(preds, rows)
    if exprs is not None:
        return M.run(exprs, kept)
    key, val = M.run([SITE["add"].expr, SITE["idiv0"].expr], kept)
    groups = {}
    for k, v in zip(key, val):
        acc = groups.setdefault(k, [None])
        if v is not None:
            acc[0] = v if acc[0] is None else acc[0] + v
    order = sorted(groups, key=lambda k: (k is None, k or 0))
    return [order, [groups[k][0] for k in order]]


def _sorted_by_key(t):
    if t is None:
        return None
    rows = sorted(zip(*[t.column(i).to_pylist() for i in range(t.num_columns)]), key=lambda r: (r[0] is None, r[0] or 0))
    return pa.table([pa.array([r[i] for r in rows], t.schema.field(i).type) for i in range(t.num_columns)], names=t.schema.names)


@pytest.mark.parametrize("name", ["filter_project", "filter_filter", "filter_aggregate", "filter_isnotnull_project"])
def test_b_rows_a_lower_filter_drops_raise_nothing(built, name):
    plan, types, preds, exprs, dead = filter_cases()[name]
    data = filter_data(name)
    rows = data.rows()
    if "null" in dead:
        for row in DEAD:
            assert not data.table().column("q")[row].is_valid and physical(data.table().column("q"), row) == 0
        unfiltered = offend_all(base(), DEAD, sites=B_SITES).rows()
    else:
        unfiltered = rows
    for s in B_SITES:      # the dropped rows offend: evaluated without the Filter (and with the operand valid) every site raises
        assert count_offenders(s, unfiltered) == len(DEAD) > 0
    run = lambda d: (_sorted_by_key if exprs is None else (lambda t: t))(_run(plan, d.table(), 2))
    check_equal(run(data), types, filter_want(name, rows))
    for k, s in enumerate(B_SITES):
        row = POS[(3 * k + len(name)) % len(POS)]
        live = offend_live(data.copy(), row, s, g=1)
        with pytest.raises(M.SparkError) as ei:
            filter_want(name, live.rows()[row:row + 1])
        assert ei.value.error_class == s.cls
        check_raises(lambda: run(live), s)


# ----------------------------------------------------------------------------------------------- (d) joins
# The probe side has 2 × 8192 + 37 rows (probe tiles of 16 × 256 and 32 × 256 rows); row n - 1 — which the lanes past the end evaluate again — is a dropped
# offender in every case.  Every (situation, path) runs as Inner, LeftOuter, LeftSemi and LeftAnti, built on the right; the path is asserted by the probe kernel
# that ran and the join_* metrics, as tests/test_join_paths_gpu.py does.  The reference is a dictionary join over the model's rows: keys of the rows that
# pass their chain's Filter, the residual condition on key-matched pairs alone.  Twelve join plans in all (three situations × four join types; the paths
# differ by the data): the first case of a situation pays their compilation — every join plan carries all the join kernels —, the others run in a second or two.

NP = 2 * 8192 + 37
JF = [I64, I32, I64, I64]                       # k, k2, v, id: a side as the join sees it
PF = [I32, I64, I64, I32, I64, I64]             # g, p, q, k2, v, id: the source of a probe chain  Filter(g = 1) → Project((p div q) + 5, k2, v, id)
BF = [I64, I64, I32, I64, I64]                  # p, q, k2, v, id: the source of a build chain  Filter(isnotnull(q) AND isnotnull(p)) → Project(the same)
POSJ = [0, 255, 256, 4095, 4096, 8191, 8192, NP - 1]
PATHS = {   # → build rows, the probe kernel of the path, the join_* metrics
    "lds": (1000, "k_jlds", dict(bucket_tables=0, direct_maps=0)),
    "chained": (10_000, "k_jprobe", dict(bucket_tables=0, direct_maps=0)),
    "bucket_scrambling": (70_000, "k_jprobe_b", dict(bucket_tables=1, mono_tables=0, direct_maps=0)),
    "direct_map": (70_000, "k_jdprobe", dict(direct_maps=1, bucket_tables=0)),
    "bucket_keymap": (70_000, "k_jprobe_bkm", dict(direct_maps=0, bucket_tables=1)),
}
PROBE_KERNELS = {"k_jlds", "k_jprobe", "k_jprobe_km", "k_jprobe_b", "k_jprobe_bkm", "k_jdprobe", "k_jprobe_bm"}
JOIN_TYPES = [S.INNER, S.LEFT_OUTER, S.LEFT_SEMI, S.LEFT_ANTI]


def _key_of(p, q):
    """(p div q) + 5 under ANSI: DIVIDE_BY_ZERO for q = 0, ARITHMETIC_OVERFLOW for a quotient above Long.MaxValue - 5"""
    return S.math("add", _idiv(p, q), S.lit(5, I64), I64, S.ANSI)


def _chain(scan, keep, p, q, rest):
    return S.project(S.filter_(scan, keep), [_key_of(p, q)] + rest)


def join_plan(situation, jt):
    keys = [S.col(0, I64)]
    left, right, cond = S.scan(JF), S.scan(JF), None
    if situation == "probe_key":
        left = _chain(S.scan(PF), S.eq(S.col(0, I32), S.lit(1, I32)), S.col(1, I64), S.col(2, I64), [S.col(3, I32), S.col(4, I64), S.col(5, I64)])
    elif situation == "build_key":
        right = _chain(S.scan(BF), S.and_(S.is_not_null(S.col(1, I64)), S.is_not_null(S.col(0, I64))), S.col(0, I64), S.col(1, I64), [S.col(2, I32), S.col(3, I64), S.col(4, I64)])
    else:      # the residual over left ++ right: (l.v div r.v) + 5 > 5
        cond = S.gt(_key_of(S.col(2, I64), S.col(6, I64)), S.lit(5, I64))
    return S.hash_join(left, right, keys, keys, jt, S.BUILD_RIGHT, cond)


def _build_keys(path, rng):
    nb = PATHS[path][0]
    if path == "lds":
        return rng.integers(10, 800, nb)
    if path == "chained":
        return rng.integers(10, 9000, nb)
    if path == "bucket_scrambling":      # every key but one would land in the monotone hash's first partition: it is refused, the scrambling hash takes over
        keys = rng.permutation(np.arange(nb, dtype=np.int64) * 2 + 1000)
        keys[5] = 1 << 40
        return keys
    keys = rng.permutation(np.arange(1000, 1000 + 3 * nb, 3, dtype=np.int64))
    if path == "bucket_keymap":
        keys[nb // 2] = keys[7]      # one key twice, far apart: the direct map is refused, the bucket table keeps the key bitmap
    return keys


class JoinData:
    """columns of the two SOURCE tables as numpy arrays with NULL masks (left = probe, right = build), per situation"""

    def __init__(self, situation, path, seed):
        rng = np.random.default_rng(seed)
        nb = PATHS[path][0]
        self.situation = situation
        bk = _build_keys(path, rng).astype(np.int64)
        # the dead rows of the build side: keys no probe row has (negative and odd: no path's keys are)
        self.dead_b = np.array(sorted({0, 255, 256, nb - 1} | set(rng.integers(300, nb - 1, 12).tolist())))      # (rows 5 and 7 carry a path's special keys)
        self.dead_p = np.array(sorted(set(POSJ) | set(rng.integers(1, NP - 1, 12).tolist())))
        live_b = np.setdiff1d(np.arange(nb), self.dead_b)
        pk = np.where(rng.random(NP) < 0.6, bk[live_b[rng.integers(0, len(live_b), NP)]], rng.integers(-(1 << 41), -(1 << 40) - 10, NP))
        sign = lambda n: rng.choice(np.array([-1, 1], np.int64), n)
        nonzero = lambda n: rng.integers(1, 1000, n) * sign(n)
        b = {"k": bk, "k2": rng.integers(0, 3, nb).astype(np.int32), "v": nonzero(nb), "id": np.arange(nb, dtype=np.int64)}
        p = {"k": pk.astype(np.int64), "k2": rng.integers(0, 3, NP).astype(np.int32), "v": nonzero(NP), "id": np.arange(NP, dtype=np.int64)}
        self.null = {"L": {}, "R": {}}
        if situation == "probe_key":
            q = sign(NP)
            p.update(g=np.ones(NP, np.int32), q=q, p=(p["k"] - 5) * q)
            p["g"][rng.random(NP) < 0.2] = 0
            for n, row in enumerate(self.dead_p):      # dropped offenders: a zero divisor, or a quotient whose + 5 overflows
                p["g"][row] = 0
                p["p"][row], p["q"][row] = (100 + n, 0) if n % 2 == 0 else (MAX64 - n, 1)
            self.null["L"]["q"] = rng.random(NP) < 0.02      # (a NULL divisor: a NULL key)
            self.null["L"]["q"][self.dead_p] = False
            self.names_l, self.names_r = ["g", "p", "q", "k2", "v", "id"], ["k", "k2", "v", "id"]
            self.null["R"]["k"] = rng.random(nb) < 0.02
        elif situation == "build_key":
            q = sign(nb)
            b.update(q=q, p=(b["k"] - 5) * q)
            self.null["R"]["q"], self.null["R"]["p"] = np.zeros(nb, bool), np.zeros(nb, bool)
            for n, row in enumerate(self.dead_b):      # NULL slots that physically hold the offender
                b["p"][row], b["q"][row] = (100 + n, 0) if n % 2 == 0 else (MAX64 - n, 1)
                self.null["R"]["q" if n % 2 == 0 else "p"][row] = True
            self.names_l, self.names_r = ["k", "k2", "v", "id"], ["p", "q", "k2", "v", "id"]
            self.null["L"]["k"] = rng.random(NP) < 0.02
            self.null["L"]["k"][NP - 1] = False
        else:
            b["k"][self.dead_b] = -2 * np.arange(1, len(self.dead_b) + 1) - 1      # keys no probe row has …
            b["v"][self.dead_b] = 0                                               # … and a zero divisor for whoever asks about the pair
            p["k"][self.dead_p] = -(1 << 50) - np.arange(len(self.dead_p))        # probe rows without a partner whose quotient + 5 overflows against v = 1
            p["v"][self.dead_p] = MAX64 - np.arange(len(self.dead_p))
            self.names_l = self.names_r = ["k", "k2", "v", "id"]
            self.null["L"]["k"] = rng.random(NP) < 0.02
            self.null["L"]["k"][self.dead_p] = False
            self.null["R"]["k"] = rng.random(nb) < 0.02
            self.null["R"]["k"][self.dead_b] = False
        self.L, self.R = p, b

    def tables(self):
        mk = lambda cols, names, null: pa.table([pa.array(cols[n], mask=null.get(n)) for n in names], names=names)
        return [mk(self.L, self.names_l, self.null["L"]), mk(self.R, self.names_r, self.null["R"])]

    def rows(self, side):
        cols, names, null = (self.L, self.names_l, self.null["L"]) if side == "L" else (self.R, self.names_r, self.null["R"])
        return list(zip(*[[None if (n in null and null[n][r]) else v for r, v in enumerate(cols[n].tolist())] for n in names]))

    def make_live(self, kind):
        """one live offender (kind 0: the zero divisor, 1: the overflow); → the site"""
        if self.situation == "probe_key":
            row = int(self.dead_p[3 + kind])
            self.L["g"][row] = 1
            self.L["p"][row], self.L["q"][row] = (77, 0) if kind == 0 else (MAX64 - 1, 1)
        elif self.situation == "build_key":
            row = int(self.dead_b[2 + kind])
            self.null["R"]["q"][row] = self.null["R"]["p"][row] = False
            self.R["p"][row], self.R["q"][row] = (77, 0) if kind == 0 else (MAX64 - 1, 1)
        else:      # ONE key-matched pair (the dead build rows' keys are unique): a dead probe row takes a dead build row's key — 12 div 0, or (MAX - n) div 1 + 5
            pr, br = int(self.dead_p[3 + kind]), int(self.dead_b[3 + kind])
            self.L["k"][pr], self.L["k2"][pr] = self.R["k"][br], self.R["k2"][br]
            if kind == 0:
                self.L["v"][pr] = 12
            else:
                self.R["v"][br] = 1
        return SITE["idiv0"] if kind == 0 else SITE["add"]


def join_reference(data, jt, eager=False):
    """the join's output rows (a sorted list of tuples) by the per-row model; eager: keys of dropped rows and the residual of unmatched pairs are evaluated too"""
    c = lambda k, t: S.col(k, t)
    key_l = M.compile_expr(_key_of(c(1, I64), c(2, I64)))
    key_r = M.compile_expr(_key_of(c(0, I64), c(1, I64)))
    resid = M.compile_expr(S.gt(_key_of(c(2, I64), c(6, I64)), S.lit(5, I64)))
    left, right = [], []
    for row in data.rows("L"):
        if data.situation == "probe_key":
            if eager:
                key_l(row)
            if row[0] == 1:
                left.append((key_l(row),) + row[3:])
        else:
            left.append(row)
    for row in data.rows("R"):
        if data.situation == "build_key":
            if eager:
                key_r(tuple(0 if v is None else v for v in row))      # (the slot's physical value)
            if row[0] is not None and row[1] is not None:
                right.append((key_r(row),) + row[2:])
        else:
            right.append(row)
    nk = 1
    index = {}
    for r in right:
        if all(v is not None for v in r[:nk]):
            index.setdefault(r[:nk], []).append(r)
    out = []
    for l in left:
        if eager and data.situation == "residual":
            resid(l + right[0])
        partners = index.get(l[:nk], []) if all(v is not None for v in l[:nk]) else []
        if data.situation == "residual":
            partners = [r for r in partners if resid(l + r) is True]
        if jt == S.INNER:
            out += [l + r for r in partners]
        elif jt == S.LEFT_OUTER:
            out += [l + r for r in partners] or [l + (None,) * 4]
        elif (jt == S.LEFT_SEMI) == bool(partners):
            out.append(l)
    return sorted(out, key=lambda r: tuple((v is None, v or 0) for v in r))


def _join_run(plan, tables, ncols):
    """→ the output's sorted rows, the join's kernels with their call counts, the metrics"""
    from tests.test_hash_join_gpu import _join_metrics
    with native.collect_kernel_times() as kt:
        got, m = _join_metrics(plan, tables, ncols)
    rows = [] if got is None else sorted(zip(*[got.column(i).to_pylist() for i in range(got.num_columns)]), key=lambda r: tuple((v is None, v or 0) for v in r))
    return rows, {k: v["calls"] for k, v in kt.times.items() if k.startswith("k_j")}, m


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("situation", ["probe_key", "build_key", "residual"])
def test_d_join_raises_only_for_rows_and_pairs_it_evaluates(built, situation, path):
    """situation "residual" holds both of the issue's residual cases: dead build rows whose keys match no probe row, build row 0 among them"""
    nb = PATHS[path][0]
    data = JoinData(situation, path, seed=len(path) * 7 + len(situation))
    assert len(data.dead_p) > 0 and len(data.dead_b) > 0 and (situation != "probe_key" or data.L["g"][NP - 1] == 0)
    if situation == "build_key":      # the NULL slots physically hold the offending divisor / dividend
        t = data.tables()[1]
        for n, row in enumerate(data.dead_b):
            name = "q" if n % 2 == 0 else "p"
            assert not t.column(name)[int(row)].is_valid and physical(t.column(name), int(row)) == (0 if n % 2 == 0 else MAX64 - n)
    with pytest.raises(M.SparkError) as ei:      # not vacuous: evaluated for dropped rows and unmatched pairs too, the join raises
        join_reference(data, S.INNER, eager=True)
    assert ei.value.error_class in ("DIVIDE_BY_ZERO", "ARITHMETIC_OVERFLOW")
    for n, jt in enumerate(JOIN_TYPES):
        plan = join_plan(situation, jt)
        ncols = 4 if jt in (S.LEFT_SEMI, S.LEFT_ANTI) else 8
        want = join_reference(data, jt)
        got, calls, m = _join_run(plan, data.tables(), ncols)
        print(situation, path, jt, calls, {k: v for k, v in m.items() if k.startswith("join_")})
        assert got == want, (jt, len(got), len(want))
        assert len(want) > 100
        explain = native.compile_plan(plan.encode())      # the chain IS fused into the join: run as a pipeline of its own, its dropped rows would test nothing
        assert situation != "probe_key" or "probe side fused" in explain, explain
        assert situation != "build_key" or ("build side fused with its chain" in explain and m["join_fused_builds"] == 1), (explain, m)
        if path in ("direct_map", "bucket_keymap") and jt in (S.LEFT_SEMI, S.LEFT_ANTI) and situation != "residual":
            # a semi / anti join without a condition over one integer key of a small range asks the key bitmap alone (a path of its own: P::pkey0 on every row)
            probe_kernel, metrics = "k_jprobe_bm", dict(bitmap_only=1, bucket_tables=0, direct_maps=0)
        else:
            probe_kernel, metrics = PATHS[path][1:]
        assert probe_kernel in calls and not (PROBE_KERNELS - {probe_kernel}) & set(calls), (jt, calls)
        for name, v in metrics.items():
            assert m["join_" + name] == v, (jt, name, m)
        live = JoinData(situation, path, seed=len(path) * 7 + len(situation))
        site = live.make_live(n % 2)
        with pytest.raises(M.SparkError) as ei:
            join_reference(live, jt)
        assert ei.value.error_class == site.cls
        with pytest.raises(native.CometQueryExecutionException) as ei:
            _join_run(plan, live.tables(), ncols)
        assert json.loads(str(ei.value))["errorClass"] == site.cls, (jt, str(ei.value))
