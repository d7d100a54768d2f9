"""var_samp / var_pop, stddev_samp / stddev_pop, covar_samp / covar_pop and corr on the GPU, checked against exact moments.

The engine keeps each moment as a count and exact Float64 sums (Σx, Σy, Σx², Σy², Σxy, products split exactly with two_prod) and finishes
mean = Σx / n and m2 = Σx² − (Σx)² / n in wide integer arithmetic (comet_device.hpp "Statistical aggregates").  So the checks are:
  * every Partial state (count, mean, m2, algo_const) within 1 ULP of the exact value of the rows, for ungrouped, LDS-table and global-table plans;
  * Final results within 2 ULP (variance, stddev, covariance) / 4 ULP (corr) of exact; grouped and ungrouped corr follow their own formulas;
  * the same bits for shuffled rows, other batch sizes and a later chunk that moves the exponent window;
  * the merge of Partial states is the exact merge of the states as they were rounded.
The data are dyadic rationals (integers / 2^K), so the exact moments are Python integers.  The reference's Welford recurrence is restated in row
order only to REPORT its distance; its result moves with batch boundaries, so no bit-equality with it is possible.
"""
import math
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import pyarrow as pa
import pytest

from datafusion_comet_amd import native, serde as S

pytestmark = pytest.mark.gpu
F64, I32 = S.T_DOUBLE, S.T_INT32
K = 4                      # values are integers / 2^K
getcontext().prec = 60


def ulp_distance(a, b) -> int:
    if a is None or b is None:
        return 0 if a is None and b is None else 1 << 62
    if math.isnan(a) or math.isnan(b):
        return 0 if (math.isnan(a) and math.isnan(b)) else 1 << 62

    def key(x):
        (i,) = np.array([x], dtype=np.float64).view(np.int64)
        i = int(i)
        return i if i >= 0 else -(i & 0x7FFFFFFFFFFFFFFF)
    return abs(key(a) - key(b))


def run(plan, table, ncols, batch_rows=8192, config=None):
    kw = {"config": S.config_map(config)} if config else {}
    out = native.execute_to_table([native.HostInput.from_table(table, batch_rows)], ncols, plan.encode(), batch_size=0, **kw)
    return pa.Table.from_batches(out) if out else None


def rows_of(t):
    return [tuple(t.column(i)[r].as_py() for i in range(t.num_columns)) for r in range(t.num_rows)]


def by_key(t):
    return {r[0]: r[1:] for r in rows_of(t)}


def data(n, ngroups, seed, nulls=False):
    """x = (X + 3·2^20) / 2^K, y = (2·X − Z) / 2^K with small integers X, Z; g in [0, ngroups)"""
    rng = np.random.default_rng(seed)
    X = rng.integers(-2**20, 2**20, n) + 3 * 2**20
    Y = 2 * X - rng.integers(-2**19, 2**19, n)
    g = rng.integers(0, max(ngroups, 1), n).astype(np.int32)
    g[:ngroups] = np.arange(ngroups)          # every group has rows
    xm = rng.random(n) < 0.05 if nulls else None
    ym = rng.random(n) < 0.05 if nulls else None
    t = pa.table({"x": pa.array(X / 2.0**K, mask=xm), "y": pa.array(Y / 2.0**K, mask=ym), "g": pa.array(g)})
    return t, X, Y, g, xm, ym


def exact_sums(X, Y, g, ngroups, keep):
    """per group: (n, Σx, Σy, Σx², Σy², Σxy) of the integers X, Y over the rows `keep`, as Python ints (no int64 sum overflows here)"""
    out = []
    X, Y, g = X[keep].astype(np.int64), Y[keep].astype(np.int64), g[keep]
    cols = []
    for v in (np.ones_like(X), X, Y):
        a = np.zeros(ngroups, np.int64)
        np.add.at(a, g, v)
        cols.append(a)
    for u, v in ((X, X), (Y, Y), (X, Y)):      # products up to 2^46, < 2^16 rows per group here … split in halves to stay exact anyway
        hi, lo = np.zeros(ngroups, np.int64), np.zeros(ngroups, np.int64)
        p_hi, p_lo = (u * v) >> 20, (u * v) & ((1 << 20) - 1)
        np.add.at(hi, g, p_hi)
        np.add.at(lo, g, p_lo)
        cols.append((hi, lo))
    for k in range(ngroups):
        n, sx, sy = int(cols[0][k]), int(cols[1][k]), int(cols[2][k])
        q = [(int(h[k]) << 20) + int(lo_[k]) for h, lo_ in cols[3:]]
        out.append((n, sx, sy, *q))
    return out


def exact_state(n, sx, sy, sxx, syy, sxy):
    """exact (count, mean1, mean2, m2_1, m2_2, c) of the values X / 2^K, Y / 2^K"""
    if n == 0:
        return (0, Fraction(0), Fraction(0), Fraction(0), Fraction(0), Fraction(0))
    d1, d2 = Fraction(1, 2**K), Fraction(1, 2**(2 * K))
    return (n, Fraction(sx, n) * d1, Fraction(sy, n) * d1, Fraction(n * sxx - sx * sx, n) * d2, Fraction(n * syy - sy * sy, n) * d2,
            Fraction(n * sxy - sx * sy, n) * d2)


def sqrt_frac(f: Fraction) -> float:
    return float((Decimal(f.numerator) / Decimal(f.denominator)).sqrt())


def exact_results(st, null_on_div0=True):
    """exact var_samp, var_pop, stddev_samp, stddev_pop, covar_samp, covar_pop, corr of one group (None = NULL)"""
    n, _, _, m2x, m2y, c = st
    nan = float("nan")
    if n == 0:
        return [None] * 7
    one = None if null_on_div0 else nan
    vs = one if n == 1 else float(m2x / (n - 1))
    sds = one if n == 1 else sqrt_frac(m2x / (n - 1))
    cs = one if n == 1 else float(c / (n - 1))
    if n == 1:
        cr = one
    elif m2x == 0 or m2y == 0:
        cr = None
    else:
        cr = math.copysign(sqrt_frac(c * c / (m2x * m2y)), float(c))
    return [vs, float(m2x / n), sds, sqrt_frac(m2x / n), cs, float(c / n), cr]


# two aggregates (one pipeline writes at most 22 output columns, a Final merge keeps at most 8 exact sums): 12 and 10 state columns
VAR_AGGS = lambda x, y, **kw: [S.variance(x, S.SAMPLE, **kw), S.variance(x, S.POPULATION, **kw), S.stddev(x, S.SAMPLE, **kw), S.stddev(x, S.POPULATION, **kw)]
PAIR_AGGS = lambda x, y, **kw: [S.covariance(x, y, S.SAMPLE, **kw), S.corr(x, y, **kw)]
STATE_WIDTH = [3, 3, 3, 3]


def partial_plan(grouped, aggs_fn=VAR_AGGS, **kw):
    x, y, g = S.col(0, F64), S.col(1, F64), S.col(2, I32)
    return S.hash_agg(S.scan([F64, F64, I32]), [g] if grouped else [], aggs_fn(x, y, **kw))


def check_states(states_row, st, label):
    """the state columns of the functions in STATE_WIDTH's order (as many as the row holds) against the exact state of one group"""
    n, m1, m2m, m2x, m2y, c = st
    pos = 0
    for f, w in enumerate(STATE_WIDTH):
        if pos >= len(states_row):
            break
        s = states_row[pos:pos + w]
        pos += w
        assert s[0] == n, (label, f, s[0], n)
        want = [float(m1), float(m2x)] if w == 3 else [float(m1), float(m2m), float(c)] + ([float(m2x), float(m2y)] if w == 6 else [])
        for got, exp in zip(s[1:], want):
            assert ulp_distance(got, exp) <= 1, f"{label}: function {f} state {s} vs exact {want}"


# --------------------------------------------------------------------------- the reference's in-file vectors

def _vec_plan(grouped, aggs):
    return S.hash_agg(S.scan([F64, F64, I32]), [S.col(2, I32)] if grouped else [], aggs)


def final_over(partial, table, ncols_partial, ncols_final, config=None):
    st = run(partial, table, ncols_partial, config=config)
    return run(S.final_of(partial, st.schema), st, ncols_final)


@pytest.mark.parametrize("grouped", [False, True])
def test_reference_vectors(built, grouped):
    x, y = S.col(0, F64), S.col(1, F64)
    ng = 1 if grouped else 0
    # variance.rs: var_pop([1..5]) = 2, var_samp = 2.5; stddev.rs: stddev_pop = sqrt(2); covariance.rs / correlation.rs: y = 2x + 1 → covar_pop = 4, corr = 1
    t = pa.table({"x": pa.array([1.0, 2.0, 3.0, 4.0, 5.0]), "y": pa.array([3.0, 5.0, 7.0, 9.0, 11.0]), "g": pa.array([7] * 5, pa.int32())})
    aggs_v = [S.variance(x, S.POPULATION), S.variance(x), S.stddev(x, S.POPULATION), S.stddev(x)]
    aggs_p = [S.covariance(x, y, S.POPULATION), S.covariance(x, y)]
    aggs_c = [S.corr(x, y)]
    assert rows_of(final_over(_vec_plan(grouped, aggs_v), t, ng + 12, ng + 4))[0][ng:] == (2.0, 2.5, math.sqrt(2.0), math.sqrt(2.5))
    corr = 1.0 if grouped else (20.0 / 5) / (math.sqrt(10.0 / 5) * math.sqrt(40.0 / 5))      # grouped c / sqrt(m2x·m2y), ungrouped covar_pop / (σx·σy)
    assert rows_of(final_over(_vec_plan(grouped, aggs_p), t, ng + 8, ng + 2))[0][ng:] == (4.0, 5.0)
    assert rows_of(final_over(_vec_plan(grouped, aggs_c), t, ng + 6, ng + 1))[0][ng:] == (corr,)
    # NULLs are ignored; multi-group; an empty group (all NULL) is NULL; a FILTER keeps its rows
    t = pa.table({"x": pa.array([1.0, None, 3.0, 10.0, 20.0, None]), "y": pa.array([1.0, 5.0, 2.0, 1.0, 2.0, 4.0]), "g": pa.array([1, 1, 1, 2, 2, 3], pa.int32())})
    if grouped:
        fin = final_over(_vec_plan(True, [S.variance(x, S.POPULATION), S.variance(x)]), t, 1 + 6, 3)
        assert by_key(fin) == {1: (1.0, 2.0), 2: (25.0, 50.0), 3: (None, None)}
    keep = S.gt(S.col(1, F64), S.lit(1.5, F64))
    fin = final_over(_vec_plan(grouped, [S.variance(x, S.POPULATION, filter=keep)]), t, ng + 3, ng + 1)
    want = {1: (0.0,), 2: (0.0,), 3: (None,)} if grouped else None
    if grouped:
        assert by_key(fin) == want
    else:
        assert rows_of(fin)[0] == (float(np.var([3.0, 20.0])),)
    # a single row: SAMPLE is NULL under null_on_divide_by_zero, NaN under the legacy setting; POPULATION is 0
    one = pa.table({"x": pa.array([4.0]), "y": pa.array([2.0]), "g": pa.array([5], pa.int32())})
    r = rows_of(final_over(_vec_plan(grouped, [S.variance(x), S.variance(x, null_on_divide_by_zero=False), S.variance(x, S.POPULATION)]), one, ng + 9, ng + 3))[0][ng:]
    r += rows_of(final_over(_vec_plan(grouped, [S.corr(x, y)]), one, ng + 6, ng + 1))[0][ng:]
    r += rows_of(final_over(_vec_plan(grouped, [S.corr(x, y, null_on_divide_by_zero=False)]), one, ng + 6, ng + 1))[0][ng:]
    assert r[0] is None and math.isnan(r[1]) and r[2] == 0.0 and r[3] is None and math.isnan(r[4])
    # merge equals single shot: two Partial outputs merged give the single-shot result
    t = pa.table({"x": pa.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]), "y": pa.array([2.0, 1.0, 4.0, 3.0, 6.0, 5.0]), "g": pa.array([0] * 6, pa.int32())})
    for aggs, w in ((aggs_v, 12), (aggs_p, 8), (aggs_c, 6)):
        p = _vec_plan(grouped, aggs)
        whole = final_over(p, t, ng + w, ng + len(aggs))
        parts = pa.concat_tables([run(p, t.slice(0, 2), ng + w), run(p, t.slice(2), ng + w)])
        merged = run(S.final_of(p, parts.schema), parts, ng + len(aggs))
        assert rows_of(merged) == rows_of(whole)


# --------------------------------------------------------------------------- Partial states and Final results against exact moments

@pytest.mark.parametrize("ngroups", [0, 5, 40_000])
def test_partial_states_and_final_results_are_exact(built, ngroups):
    n = 400_000
    t, X, Y, g, xm, ym = data(n, ngroups, 10 + ngroups, nulls=True)
    ng = 1 if ngroups else 0
    pv, pp = partial_plan(ngroups > 0), partial_plan(ngroups > 0, PAIR_AGGS)
    stv, stp = run(pv, t, ng + 12), run(pp, t, ng + 10)
    groups = max(ngroups, 1)
    gg = g if ngroups else np.zeros(n, np.int32)
    only_x = exact_sums(X, Y, gg, groups, ~xm)
    both = exact_sums(X, Y, gg, groups, ~xm & ~ym)
    keyed = lambda tb: by_key(tb) if ngroups else {0: rows_of(tb)[0]}
    gv, gp = keyed(stv), keyed(stp)
    assert len(gv) == len(gp) == groups
    for k in range(groups):
        # variance / stddev see the rows where x is valid; covariance / corr those where both are
        check_states(gv[k], exact_state(*only_x[k]), f"group {k}")
        n2, m1, m2m, m2x, m2y, c = exact_state(*both[k])
        cov, cor = gp[k][0:4], gp[k][4:10]
        assert cov[0] == n2 and cor[0] == n2
        for got_v, exp in zip(list(cov[1:]) + list(cor[1:]), [m1, m2m, c] * 2 + [m2x, m2y]):
            assert ulp_distance(got_v, float(exp)) <= 1, (k, cov, cor)
    fv, fp = keyed(run(S.final_of(pv, stv.schema), stv, ng + 4)), keyed(run(S.final_of(pp, stp.schema), stp, ng + 2))
    res = {k: fv[k] + fp[k] for k in range(groups)}
    for k in range(groups):
        ex_x, ex_b = exact_results(exact_state(*only_x[k])), exact_results(exact_state(*both[k]))
        want = ex_x[:4] + [ex_b[4], ex_b[6]]
        for f, (gv_, wv) in enumerate(zip(res[k], want)):
            assert ulp_distance(gv_, wv) <= (4 if f == 5 else 2), (k, f, gv_, wv)


def test_corr_follows_the_grouped_and_ungrouped_formulas(built):
    """Final over one Partial state per group reproduces mean and m2 bit for bit (the merge is exact), so the result is the formula applied to the
    state: grouped c / sqrt(m2_1 · m2_2), ungrouped covar_pop / (stddev_pop1 · stddev_pop2)"""
    t, *_ = data(50_000, 3, 77)
    for grouped in (False, True):
        ng = 1 if grouped else 0
        p = partial_plan(grouped, lambda x, y: [S.corr(x, y)])
        st = run(p, t, ng + 6)
        fin = run(S.final_of(p, st.schema), st, ng + 1)
        for srow, frow in zip(sorted(rows_of(st)), sorted(rows_of(fin))):
            n, _, _, c, m2x, m2y = srow[ng:]
            want = c / math.sqrt(m2x * m2y) if grouped else (c / n) / (math.sqrt(m2x / n) * math.sqrt(m2y / n))
            assert frow[ng] == want, (grouped, srow, frow, want)


# --------------------------------------------------------------------------- order independence

def test_same_bits_for_any_order_batching_and_window(built):
    t, X, Y, g, _, _ = data(300_000, 5, 21)
    p = partial_plan(True, lambda x, y: VAR_AGGS(x, y)[:2] + PAIR_AGGS(x, y))      # var, covar, corr: 3 + 3 + 4 + 6 state columns
    base = by_key(run(p, t, 17))
    rng = np.random.default_rng(5)
    perm = rng.permutation(t.num_rows)
    shuffled = t.take(pa.array(perm))
    assert by_key(run(p, shuffled, 17, batch_rows=1000)) == base
    assert by_key(run(p, shuffled, 17, batch_rows=1 << 20)) == base
    # a later chunk 2^40 larger: Σx²'s window moves up from its default after the first chunk has been accumulated (the earlier accumulators are
    # shifted, no bit is lost) — the same bits as one pass over everything
    big = pa.table({"x": pa.array(np.asarray(t.column(0)) * 2.0**40), "y": pa.array(np.asarray(t.column(1)) * 2.0**40), "g": t.column(2)})
    both = pa.concat_tables([t, big])
    cfg = {"spark.comet.gpu.chunkRows": 65536}
    for q, nc, rows in ((p, 17, by_key), (partial_plan(False, lambda x, y: VAR_AGGS(x, y)[:2] + PAIR_AGGS(x, y)), 16, rows_of)):
        assert rows(run(q, both, nc, batch_rows=65536, config=cfg)) == rows(run(q, both, nc, batch_rows=1 << 20))


# --------------------------------------------------------------------------- Partial → Final, Partial → PartialMerge → Final

def exact_merge(states, width):
    """the exact merge of rounded Welford states (count, mean1[, mean2], c / m2 …) → exact (n, mean1, mean2, c, m2_1, m2_2) as Fractions"""
    N = sum(int(s[0]) for s in states)
    S1 = sum(Fraction(s[0]) * Fraction(s[1]) for s in states)
    if width == 3:
        S2 = sum(Fraction(s[2]) + Fraction(s[0]) * Fraction(s[1]) ** 2 for s in states)
        return N, S1 / N, None, S2 - S1 * S1 / N
    S1y = sum(Fraction(s[0]) * Fraction(s[2]) for s in states)
    C = sum(Fraction(s[3]) + Fraction(s[0]) * Fraction(s[1]) * Fraction(s[2]) for s in states)
    return N, S1 / N, S1y / N, C - S1 * S1y / N


def test_partial_final_and_partial_merge(built):
    t, X, Y, g, _, _ = data(240_000, 4, 31)
    x, y = S.col(0, F64), S.col(1, F64)
    p = S.hash_agg(S.scan([F64, F64, I32]), [S.col(2, I32)], [S.variance(x), S.covariance(x, y), S.avg(x, F64, F64), S.sum_(x, F64)])
    ncols = 1 + 3 + 4 + 2 + 1
    parts = [run(p, t.slice(i * 60_000, 60_000), ncols) for i in range(4)]
    shuffled = pa.concat_tables(parts)            # what the Final stage reads after the exchange
    fin = by_key(run(S.final_of(p, shuffled.schema), shuffled, 5))
    # PartialMerge of the first two outputs, then Final over (merged ++ the other two)
    fields = [S.from_arrow_type(f.type) for f in shuffled.schema]
    pm = S.hash_agg(S.scan(fields), [S.col(0, I32)], p.aggs, S.PARTIAL_MERGE)
    merged = run(pm, pa.concat_tables(parts[:2]), ncols)
    assert merged.schema.types == shuffled.schema.types
    fin2 = by_key(run(S.final_of(p, shuffled.schema), pa.concat_tables([merged] + parts[2:]), 5))
    whole = exact_sums(X, Y, g, 4, np.ones(len(X), bool))
    srows = rows_of(shuffled)
    for k in range(4):
        states = [r for r in srows if r[0] == k]
        _, _, _, m2 = exact_merge([s[1:4] for s in states], 3)
        N, _, _, c = exact_merge([s[4:8] for s in states], 4)
        got = fin[k]
        # within 2 ULP of the exact merge of the states the Partial stage emitted …
        assert ulp_distance(got[0], float(m2 / (N - 1))) <= 2 and ulp_distance(got[1], float(c / (N - 1))) <= 2, (k, got)
        # … and of the whole data's exact value, on both routes
        ex = exact_results(exact_state(*whole[k]))
        for gv_, wv in zip(got[:2] + fin2[k][:2], [ex[0], ex[4]] * 2):
            assert abs(gv_ - wv) <= 1e-12 * abs(wv), (k, gv_, wv)
        # avg(x) and sum(x) next to them (Σx and the count shared in the Partial stage): exact
        total = math.fsum((X[g == k] / 2.0**K).tolist())
        assert got[3] == fin2[k][3] == total and got[2] == total / int((g == k).sum())


# --------------------------------------------------------------------------- a join-fed aggregate (TPC-DS Q17's shape)

def test_stddev_above_a_hash_join(built):
    rng = np.random.default_rng(17)
    nf, nd = 200_000, 1000
    fact = pa.table({"k": pa.array(rng.integers(0, 2 * nd, nf).astype(np.int32)), "q": pa.array(rng.integers(1, 100, nf) / 4.0)})
    dim = pa.table({"k": pa.array(np.arange(nd, dtype=np.int32)), "grp": pa.array((np.arange(nd) % 7).astype(np.int32))})
    j = S.hash_join(S.scan([I32, F64]), S.scan([I32, I32]), [S.col(0, I32)], [S.col(0, I32)], S.INNER, S.BUILD_RIGHT)
    q = S.col(1, F64)
    plan = S.hash_agg(j, [S.col(3, I32)], [S.stddev(q), S.avg(q, F64, F64), S.count(q)])
    out = native.execute_to_table([native.HostInput.from_table(fact), native.HostInput.from_table(dim)], 1 + 3 + 2 + 1, plan.encode(), batch_size=0)
    got = by_key(pa.Table.from_batches(out))
    keys, qs = np.asarray(fact.column(0)), np.asarray(fact.column(1))
    hit = keys < nd
    grp = keys[hit] % 7
    Q = (qs[hit] * 4).astype(np.int64)
    for k in range(7):
        v = Q[grp == k]
        n, s1, s2 = len(v), int(v.sum()), int((v * v).sum())
        mean, m2 = Fraction(s1, n * 4), Fraction(n * s2 - s1 * s1, n * 16)
        r = got[k]
        assert r[0] == n and ulp_distance(r[1], float(mean)) <= 1 and ulp_distance(r[2], float(m2)) <= 1
        assert r[3] == math.fsum((v / 4.0).tolist()) and r[4] == n and r[5] == n


# --------------------------------------------------------------------------- edge cases

def test_edge_cases(built):
    x, y = S.col(0, F64), S.col(1, F64)
    nan, inf = float("nan"), float("inf")
    t = pa.table({"x": pa.array([None, None, 5.0, 1.0, 2.0, 4.0, 1.0, 2.0, 3.0, 1.0, nan, 2.0, inf, 1.0, 2.0, -inf, 8.0]),
                  "y": pa.array([1.0, 2.0, 6.0, 1.0, None, 3.0, 7.0, 7.0, 7.0, 1.0, 1.0, 2.0, 2.0, 1.0, 2.0, 3.0, 1.0]),
                  "g": pa.array([0, 0, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5, 6, 6], pa.int32())})
    p = S.hash_agg(S.scan([F64, F64, I32]), [S.col(2, I32)], [S.variance(x), S.variance(x, null_on_divide_by_zero=False), S.covariance(x, y, S.POPULATION), S.corr(x, y)])
    st = by_key(run(p, t, 1 + 3 + 3 + 4 + 6))
    assert st[0][:3] == (0.0, 0.0, 0.0)                            # all NULL: state (0, 0, 0)
    fin = {}
    for aggs, w in (([S.variance(x), S.variance(x, null_on_divide_by_zero=False)], 6), ([S.covariance(x, y, S.POPULATION)], 4), ([S.corr(x, y)], 6)):
        part = by_key(final_over(S.hash_agg(S.scan([F64, F64, I32]), [S.col(2, I32)], aggs), t, 1 + w, 1 + len(aggs)))
        fin = {k: fin.get(k, ()) + v for k, v in part.items()}
    assert fin[0] == (None, None, None, None)                      # … and NULL results
    assert fin[1][0] is None and math.isnan(fin[1][1])             # one row: NULL / NaN
    # covariance and corr skip rows where one side is NULL: group 2 pairs (1, 1), (4, 3)
    assert fin[2][2] == 1.5 and fin[2][3] == 1.0
    assert fin[3][3] is None                                       # corr with a constant column
    for k in (4, 5, 6):                                            # NaN, ±inf inputs: NaN results
        assert all(math.isnan(v) for v in fin[k]), (k, fin[k])
    # FILTER (WHERE y > 1.5)
    keep = S.gt(y, S.lit(1.5, F64))
    pf = S.hash_agg(S.scan([F64, F64, I32]), [S.col(2, I32)], [S.variance(x, S.POPULATION, filter=keep)])
    f = by_key(final_over(pf, t, 1 + 3, 1 + 1))
    assert f[3] == (float(np.var([1.0, 2.0, 3.0])),) and f[2] == (0.0,) and f[1] == (0.0,)


# --------------------------------------------------------------------------- ill-conditioned data

def welford(xs):
    n, mean, m2 = 0.0, 0.0, 0.0
    for v in xs:
        n += 1.0
        d1 = v - mean
        mean = d1 / n + mean
        m2 += d1 * (v - mean)
    return n, mean, m2


def test_ill_conditioned_data(built):
    x = S.col(0, F64)
    p = S.hash_agg(S.scan([F64, F64, I32]), [], [S.variance(x), S.stddev(x, S.POPULATION)])
    rng = np.random.default_rng(9)
    cases = {
        "2^30 + j/2": [2.0**30 + j / 2 for j in range(8)],
        "prices ~1e9, cents": (1e9 + rng.integers(0, 10_000, 20_000) / 100.0).tolist(),
    }
    for label, xs in cases.items():
        t = pa.table({"x": pa.array(xs), "y": pa.array(xs), "g": pa.array(np.zeros(len(xs), np.int32))})
        st = rows_of(run(p, t, 6))[0]
        fr = [Fraction(v) for v in xs]
        n = len(fr)
        s1, s2 = sum(fr), sum(v * v for v in fr)
        mean, m2 = s1 / n, s2 - s1 * s1 / n
        assert st[0] == n and ulp_distance(st[1], float(mean)) <= 1 and ulp_distance(st[2], float(m2)) <= 1, (label, st)
        fin = rows_of(final_over(p, t, 6, 2))[0]
        assert ulp_distance(fin[0], float(m2 / (n - 1))) <= 2, (label, fin)
        assert ulp_distance(fin[1], sqrt_frac(m2 / n)) <= 2, (label, fin)
        _, _, wm2 = welford(xs)
        print(f"{label}: the reference's row-order Welford m2 is {ulp_distance(wm2, float(m2))} ULP from exact, ours {ulp_distance(st[2], float(m2))}")
