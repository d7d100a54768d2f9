"""A per-row model of the expressions tests/test_dead_rows_gpu.py uses: Python ints (a decimal is its unscaled integer), floats, strs and bools, one row at a
time, NULL = None.  It restates Spark's ANSI semantics from their definitions and shares no code with oracle/oracle.py (which tests/test_dead_rows_cpu.py checks
against it) nor with the generator.

Evaluation order is what the engine must reproduce: a conditional evaluates, for a row, only what that row reaches — `If` its condition and the picked side;
`CaseWhen` the WHENs up to the first TRUE one, that one's THEN, or all WHENs and the ELSE; coalesce its arguments up to the first that is not NULL.  A raise
under a NULL operand does not happen: the operation is not evaluated for that row.  With eager=True every child of a conditional is evaluated before the choice
is made — the behaviour the tests must be able to tell from the lazy one (a case in which the eager model does not raise tests nothing)."""
import math
import re

from datafusion_comet_amd import serde as S

INTS = {S.INT8: 8, S.INT16: 16, S.INT32: 32, S.INT64: 64}


class SparkError(Exception):
    """error_class: Spark's error class; value: the offending value where the error names one (a Python value; the test formats it), else None"""

    def __init__(self, error_class, value=None):
        super().__init__(error_class)
        self.error_class = error_class
        self.value = value


def _half_up_div(num, den):
    """num / den rounded half away from zero (den > 0)"""
    q = (2 * abs(num) + den) // (2 * den)
    return -q if num < 0 else q


def _trunc_div(a, b):
    q = abs(a) // abs(b)
    return -q if (a < 0) != (b < 0) else q


def type_of(e):
    """the static type of an expression (the kinds the model knows)"""
    k = e.kind
    if k in ("bound", "literal", "cast", "check_overflow"):
        return e.dtype
    if k in ("eq", "neq", "lt", "lt_eq", "gt", "gt_eq", "is_null", "is_not_null", "not_", "and_", "or_"):
        return S.T_BOOL
    if k in ("add", "subtract", "multiply", "divide", "remainder", "integral_divide"):
        a, b = type_of(e.children[0]), type_of(e.children[1])
        if a.type_id == S.DECIMAL and k in ("add", "subtract", "multiply") and not _wide(k, a, b):
            # the exact result's type, as arrow-arith's decimal kernels give it (a CheckOverflow above brings it to Spark's)
            if k == "multiply":
                return S.decimal(min(38, a.precision + b.precision + 1), a.scale + b.scale)
            sm = max(a.scale, b.scale)
            return S.decimal(min(38, max(a.precision - a.scale, b.precision - b.scale) + sm + 1), sm)
        return e.dtype
    if k == "unary_minus":
        return type_of(e.children[0])
    if k == "if_":
        return type_of(e.children[1])
    if k == "case_when":
        return type_of(e.children[e.index])
    if k == "scalar_func":
        return e.dtype if e.dtype is not None else type_of(e.children[0])
    raise NotImplementedError(k)


def _wide(k, a, b):
    """planner.rs:1000-1008: the sums and products that are computed in 256 bits and brought to the declared type"""
    if k == "multiply":
        return a.precision + b.precision >= 38
    return max(a.scale, b.scale) + max(a.precision - a.scale, b.precision - b.scale) >= 38


def compile_expr(e, eager=False):
    """→ f(row) → value | None, raising SparkError"""
    k = e.kind
    kids = [compile_expr(c, eager) for c in e.children]
    if k == "bound":
        i = e.index
        return lambda row: row[i]
    if k == "literal":
        v = e.value
        return lambda row: v
    if k in ("eq", "neq", "lt", "lt_eq", "gt", "gt_eq"):
        import operator
        op = {"eq": operator.eq, "neq": operator.ne, "lt": operator.lt, "lt_eq": operator.le, "gt": operator.gt, "gt_eq": operator.ge}[k]
        a, b = kids

        def cmp(row):
            x, y = a(row), b(row)
            return None if x is None or y is None else op(x, y)
        return cmp
    if k in ("and_", "or_"):      # both sides are evaluated for every row (no short circuit, as in the reference); Kleene logic
        a, b = kids

        def logic(row):
            x, y = a(row), b(row)
            if k == "and_":
                return False if x is False or y is False else (None if x is None or y is None else True)
            return True if x is True or y is True else (None if x is None or y is None else False)
        return logic
    if k == "is_null":
        return lambda row: kids[0](row) is None
    if k == "is_not_null":
        return lambda row: kids[0](row) is not None
    if k == "not_":
        def not_(row):
            x = kids[0](row)
            return None if x is None else not x
        return not_
    if k == "if_":
        c, t, f = kids

        def if_(row):
            if eager:
                cv, tv, fv = c(row), t(row), f(row)
                return tv if cv is True else fv
            return t(row) if c(row) is True else f(row)
        return if_
    if k == "case_when":
        n = e.index
        whens, thens, else_ = kids[:n], kids[n:2 * n], kids[2 * n] if len(kids) > 2 * n else None

        def case_when(row):
            if eager:
                wv, tv = [w(row) for w in whens], [t(row) for t in thens]
                ev = else_(row) if else_ else None
                for w, t in zip(wv, tv):
                    if w is True:
                        return t
                return ev
            for w, t in zip(whens, thens):
                if w(row) is True:
                    return t(row)
            return else_(row) if else_ else None
        return case_when
    if k == "scalar_func" and e.value == "coalesce":
        def coalesce(row):
            if eager:
                vals = [a(row) for a in kids]
                return next((v for v in vals if v is not None), None)
            for a in kids:
                v = a(row)
                if v is not None:
                    return v
            return None
        return coalesce
    if k == "scalar_func" and e.value == "abs":
        t = type_of(e.children[0])
        ansi = len(e.children) > 1 and bool(e.children[1].value)
        lo = -(1 << (INTS[t.type_id] - 1))

        def abs_(row):
            x = kids[0](row)
            if x is None:
                return None
            if x == lo:
                if ansi:
                    raise SparkError("ARITHMETIC_OVERFLOW")
                return lo
            return abs(x)
        return abs_
    if k == "unary_minus":
        t = type_of(e.children[0])
        lo = -(1 << (INTS[t.type_id] - 1))

        def neg(row):
            x = kids[0](row)
            if x is None:
                return None
            if x == lo:
                if e.fail_on_error:
                    raise SparkError("ARITHMETIC_OVERFLOW")
                return lo
            return -x
        return neg
    if k == "check_overflow":
        bound = 10 ** e.dtype.precision - 1

        def check_overflow(row):
            x = kids[0](row)
            if x is None:
                return None
            if abs(x) > bound:
                if e.fail_on_error:
                    raise SparkError("NUMERIC_VALUE_OUT_OF_RANGE.WITH_SUGGESTION", x)
                return None
            return x
        assert type_of(e.children[0]).scale == e.dtype.scale, "the model's CheckOverflow does not rescale"
        return check_overflow
    if k == "cast":
        return _cast(e, kids[0])
    if k in ("add", "subtract", "multiply", "divide", "remainder", "integral_divide"):
        return _arith(e, kids[0], kids[1])
    raise NotImplementedError(k)


def _cast(e, child):
    src, to = type_of(e.children[0]), e.dtype
    ansi = e.eval_mode == S.ANSI
    st, tt = src.type_id, to.type_id

    def wrap(f):
        def cast(row):
            x = child(row)
            return None if x is None else f(x)
        return cast

    if st in INTS and tt in INTS:
        bits = INTS[tt]

        def int_to_int(x):
            if -(1 << (bits - 1)) <= x < (1 << (bits - 1)):
                return x
            if ansi:
                raise SparkError("CAST_OVERFLOW", x)
            x &= (1 << bits) - 1
            return x - (1 << bits) if x >> (bits - 1) else x
        return wrap(int_to_int)
    if st == S.DOUBLE and tt == S.INT64:
        assert ansi, "the model casts Float64 to Int64 under ANSI only"

        def f64_to_i64(x):
            if math.isnan(x) or abs(x) >= 2.0 ** 63:
                raise SparkError("CAST_OVERFLOW", x)
            return int(x)
        return wrap(f64_to_i64)
    if st in INTS and tt == S.DECIMAL:
        bound = 10 ** to.precision - 1

        def int_to_dec(x):
            v = x * 10 ** to.scale
            if abs(v) > bound:
                if ansi:
                    raise SparkError("NUMERIC_VALUE_OUT_OF_RANGE.WITH_SUGGESTION", x)
                return None
            return v
        return wrap(int_to_dec)
    if st == S.DECIMAL and tt == S.INT64:
        assert not ansi, "the model casts decimals to Int64 in LEGACY mode only (as CometIntegralDivide does, behind a CheckOverflow)"

        def dec_to_i64(x):
            v = _trunc_div(x, 10 ** src.scale) & ((1 << 64) - 1)
            return v - (1 << 64) if v >> 63 else v
        return wrap(dec_to_i64)
    if st == S.STRING and tt in INTS:
        assert ansi, "the model casts strings under ANSI only"
        bits = INTS[tt]

        def str_to_int(x):
            t = x.strip()
            if re.fullmatch(r"[+-]?[0-9]+", t) and -(1 << (bits - 1)) <= int(t) < (1 << (bits - 1)):
                return int(t)
            raise SparkError("CAST_INVALID_INPUT", x)
        return wrap(str_to_int)
    raise NotImplementedError(f"cast {src} -> {to}")


def _arith(e, a, b):
    k, ansi = e.kind, e.eval_mode == S.ANSI
    ta, tb = type_of(e.children[0]), type_of(e.children[1])

    def wrap(f):
        def arith(row):
            x = a(row)
            y = b(row)
            return None if x is None or y is None else f(x, y)
        return arith

    if ta.type_id in INTS:
        assert ansi, "the model's integer arithmetic is ANSI"
        bits = INTS[e.dtype.type_id]
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        if k == "remainder":
            def rem(x, y):
                if y == 0:
                    raise SparkError("REMAINDER_BY_ZERO")
                r = abs(x) % abs(y)
                return -r if x < 0 else r
            return wrap(rem)
        import operator
        op = {"add": operator.add, "subtract": operator.sub, "multiply": operator.mul}[k]

        def checked(x, y):
            v = op(x, y)
            if not lo <= v <= hi:
                raise SparkError("ARITHMETIC_OVERFLOW")
            return v
        return wrap(checked)
    assert ta.type_id == S.DECIMAL and tb.type_id == S.DECIMAL
    s1, s2 = ta.scale, tb.scale
    if k in ("divide", "integral_divide"):
        s3 = e.dtype.scale
        up = s3 - s1 + s2      # the quotient of the unscaled values carries scale s1 - s2: 10^up brings it to s3
        assert up >= 0
        check_long = k == "integral_divide" and e.check_divide_overflow and ansi

        def div(x, y):
            if y == 0:
                if ansi:
                    raise SparkError("DIVIDE_BY_ZERO")
                return None
            if k == "integral_divide":
                q = _trunc_div(x * 10 ** s2, y * 10 ** s1)      # the whole part of the quotient of the VALUES
                if check_long and not -(1 << 63) <= q < (1 << 63):
                    raise SparkError("ARITHMETIC_OVERFLOW")
                return q
            q = _half_up_div(x * 10 ** up, abs(y))
            return -q if y < 0 else q
        return wrap(div)
    if k == "remainder":
        sm = max(s1, s2)

        def drem(x, y):
            if y == 0:
                if ansi:
                    raise SparkError("REMAINDER_BY_ZERO")
                return None
            x, y = x * 10 ** (sm - s1), y * 10 ** (sm - s2)
            r = abs(x) % abs(y)
            return -r if x < 0 else r
        return wrap(drem)
    sm = max(s1, s2)
    if _wide(k, ta, tb):
        bound = 10 ** e.dtype.precision - 1
        down = (s1 + s2 if k == "multiply" else sm) - e.dtype.scale
        assert down >= 0

        def wide(x, y):
            v = x * y if k == "multiply" else (x * 10 ** (sm - s1) + (y if k == "add" else -y) * 10 ** (sm - s2))
            if down:
                v = _half_up_div(v, 10 ** down)
            if abs(v) > bound:
                if ansi:
                    raise SparkError("ARITHMETIC_OVERFLOW")
                return None
            return v
        return wrap(wide)
    if k == "multiply":
        return wrap(lambda x, y: x * y)
    return wrap(lambda x, y: x * 10 ** (sm - s1) + (y if k == "add" else -y) * 10 ** (sm - s2))


def run(exprs, rows, eager=False):
    """every expression over every row, row by row → one list per expression (raises the first SparkError met)"""
    fs = [compile_expr(e, eager) for e in exprs]
    out = [[None] * len(rows) for _ in fs]
    for r, row in enumerate(rows):
        for c, f in enumerate(fs):
            out[c][r] = f(row)
    return out


def error_of(exprs, rows, eager=False):
    """the SparkError the rows raise, or None"""
    try:
        run(exprs, rows, eager)
    except SparkError as err:
        return err
    return None
