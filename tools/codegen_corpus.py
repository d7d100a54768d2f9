#!/usr/bin/env python3
"""A fixed corpus of plans and what the pipeline generator makes of each, without a GPU: per plan, the SHA-256 of the whole comet_plan_codegen JSON (kernel
source, kernels, output descriptors, fix_sums, R) with every input column's validity off and on, and comet_check_plan's text.  A refused plan is recorded with its
refusal.  tests/golden/codegen_corpus.json is this tool's output at the commit before the generator was restructured; tests/test_codegen_corpus_cpu.py compares.

  python tools/codegen_corpus.py [--out f.json]      (no COMET_* generator variable set)"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from datafusion_comet_amd import native, serde as S, tpch  # noqa: E402

B, I8, I16, I32, I64, F32, F64, STR = S.T_BOOL, S.T_INT8, S.T_INT16, S.T_INT32, S.T_INT64, S.T_FLOAT, S.T_DOUBLE, S.T_STRING
DATE, TS, TS_NTZ = S.T_DATE, S.T_TIMESTAMP, S.DataType(S.TIMESTAMP_NTZ)
D12, D18, D22, D38 = S.decimal(12, 2), S.decimal(18, 3), S.decimal(22, 2), S.decimal(38, 4)
CTX = dict(sql_text="select sum(x) from t", start_index=7, stop_index=12, line=1, start_position=7)

# the scan every Partial plan reads: key, then one column of each value type
FIELDS = [I32, I64, F64, D12, D38, I8, F64, F32, I32, DATE, B, I16]
K, X, F, DD12, DD38, BY, G, FF, XI, DT, BO, SH = [S.col(i, t) for i, t in enumerate(FIELDS)]
FLT = S.gt(X, S.lit(0, I64))


def filtered(agg):
    agg.filter = FLT
    return agg


def aggregate_kinds():
    """name → (make the AggExpr, the types of its Partial state columns, whether a FILTER variant is recorded)"""
    avg_d12 = lambda mode=S.LEGACY: S.avg(DD12, S.decimal(16, 6), D22, mode)
    avg_d38 = lambda mode=S.LEGACY: S.avg(DD38, S.decimal(38, 8), D38, mode)
    kinds = {
        "count": (lambda: S.count(X), [I64], True),
        "count_3": (lambda: S.count(X, F, DD12), [I64], True),
        "count_lit": (lambda: S.count(S.lit(1, I32)), [I64], False),
        "sum_i32": (lambda: S.sum_(XI, I64), [I64], False),
        "sum_i64": (lambda: S.sum_(X, I64), [I64], True),
        "sum_f32": (lambda: S.sum_(FF, F64), [F64], False),
        "sum_f64": (lambda: S.sum_(F, F64), [F64], True),
        "avg_i64": (lambda: S.avg(X, F64, F64), [F64, I64], False),
        "avg_f32": (lambda: S.avg(FF, F64, F64), [F64, I64], False),
        "avg_f64": (lambda: S.avg(F, F64, F64), [F64, I64], True),
        "sum_d12": (lambda: S.sum_(DD12, D22), [D22, B], True),                      # static bound: Sum128
        "sum_d12_ansi": (lambda: S.sum_(DD12, D22, S.ANSI), [D22, B], False),
        "sum_d38": (lambda: S.sum_(DD38, D38), [D38, B], True),                      # dynamic: Sum192 and the overflow words
        "sum_d38_ansi": (lambda: S.sum_(DD38, D38, S.ANSI), [D38, B], True),
        "sum_d38_ansi_ctx": (lambda: S.with_context(S.sum_(DD38, D38, S.ANSI), 3, **CTX), [D38, B], False),
        "sum_d38_try": (lambda: S.sum_(DD38, D38, S.TRY), [D38, B], False),
        "avg_d12": (lambda: avg_d12(), [D22, I64], True),
        "avg_d12_ansi": (lambda: avg_d12(S.ANSI), [D22, I64], False),
        "avg_d38": (lambda: avg_d38(), [D38, I64], True),
        "avg_d38_ansi": (lambda: avg_d38(S.ANSI), [D38, I64], False),
        "avg_d38_ansi_ctx": (lambda: S.with_context(avg_d38(S.ANSI), 4, **CTX), [D38, I64], False),
        "min_i32": (lambda: S.min_(XI, I32), [I32], False),
        "max_i64": (lambda: S.max_(X, I64), [I64], True),
        "min_f32": (lambda: S.min_(FF, F32), [F32], False),
        "max_f64": (lambda: S.max_(F, F64), [F64], True),
        "min_d12": (lambda: S.min_(DD12, D12), [D12], True),
        "max_d38": (lambda: S.max_(DD38, D38), [D38], False),                        # grouped: refused
        "min_date": (lambda: S.min_(DT, DATE), [DATE], False),
        "var_samp": (lambda: S.variance(F), [F64] * 3, True),
        "var_pop": (lambda: S.variance(F, S.POPULATION), [F64] * 3, False),
        "stddev_samp": (lambda: S.stddev(F, S.SAMPLE, False), [F64] * 3, False),
        "stddev_pop": (lambda: S.stddev(F, S.POPULATION), [F64] * 3, True),
        "covar_samp": (lambda: S.covariance(F, G), [F64] * 4, True),
        "covar_pop": (lambda: S.covariance(F, G, S.POPULATION), [F64] * 4, False),
        "corr": (lambda: S.corr(F, G), [F64] * 6, True),
        "corr_legacy": (lambda: S.corr(F, G, False), [F64] * 6, False),
        "first_i64": (lambda: S.first_(X, I64), [I64, B], True),
        "first_bool_nn": (lambda: S.first_(BO, B, True), [B, B], False),
        "first_f32": (lambda: S.first_(FF, F32), [F32, B], False),
        "last_f64": (lambda: S.last_(F, F64), [F64, B], False),
        "last_d12_nn": (lambda: S.last_(DD12, D12, True), [D12, B], True),
        "last_d38_nn": (lambda: S.last_(DD38, D38, True), [D38, B], True),
        "bit_and_i8": (lambda: S.bit_and_agg(BY, I8), [I8], True),
        "bit_or_i16": (lambda: S.bit_or_agg(SH, I16), [I16], False),
        "bit_xor_i64": (lambda: S.bit_xor_agg(X, I64), [I64], True),
    }
    return kinds


def state_plan(agg, state, grouped, mode):
    sf = ([I32] if grouped else []) + state
    return S.hash_agg(S.scan(sf), [S.col(0, I32)] if grouped else [], [agg], mode)


def aggregate_plans():
    for name, (mk, state, with_filter) in aggregate_kinds().items():
        for grouped in (False, True):
            g = "grouped" if grouped else "ungrouped"
            keys = [K] if grouped else []
            yield f"agg/{name}/partial/{g}", S.hash_agg(S.scan(FIELDS), keys, [mk()])
            if with_filter:
                yield f"agg/{name}/partial_filter/{g}", S.hash_agg(S.scan(FIELDS), keys, [filtered(mk())])
            yield f"agg/{name}/final/{g}", state_plan(mk(), state, grouped, S.FINAL)
            yield f"agg/{name}/partial_merge/{g}", state_plan(mk(), state, grouped, S.PARTIAL_MERGE)


def shared_and_mixed_plans():
    for grouped in (False, True):
        g = "grouped" if grouped else "ungrouped"
        keys = [K] if grouped else []
        yield f"shared/avg_var_stddev/{g}", S.hash_agg(S.scan(FIELDS), keys, [S.avg(F, F64, F64), S.variance(F), S.stddev(F), S.sum_(F, F64)])
        yield f"shared/min_bitxor_bitor/{g}", S.hash_agg(S.scan(FIELDS), keys, [S.bit_xor_agg(X, I64), S.min_(X, I64), S.bit_or_agg(X, I64), S.count(X)])
        yield f"shared/sum_avg_d38/{g}", S.hash_agg(S.scan(FIELDS), keys, [S.sum_(DD38, D38), S.avg(DD38, S.decimal(38, 8), D38), S.count(DD38), S.sum_(DD38, D38, S.ANSI)])
        yield f"shared/corr_covar_var/{g}", S.hash_agg(S.scan(FIELDS), keys, [S.corr(F, G), S.covariance(F, G), filtered(S.variance(G))])
        yield f"shared/first_last_same/{g}", S.hash_agg(S.scan(FIELDS), keys, [S.first_(X, I64), S.first_(X, I64), S.last_(X, I64), S.last_(X, I64, True), S.first_(DD38, D38)])
        many = [S.first_(X, I64), S.last_(F, F64, True), S.bit_and_agg(BY, I8), S.count(X), S.sum_(DD38, D38), S.avg(DD12, S.decimal(16, 6), D22), S.min_(F, F64),
                S.max_(DD12, D12), S.sum_(XI, I64), S.stddev(G), filtered(S.sum_(F, F64))]
        yield f"shared/one_of_each/{g}", S.hash_agg(S.scan(FIELDS), keys, many)
        ctx2 = dict(CTX, start_index=20, stop_index=25)
        yield f"shared/two_contexts/{g}", S.hash_agg(S.scan(FIELDS), keys, [S.with_context(S.sum_(DD38, D38, S.ANSI), 3, **CTX), S.with_context(S.sum_(S.cast(DD12, D38), D38, S.ANSI), 4, **ctx2)])
        # mixed modes (the count(DISTINCT) rewrite): PartialMerge aggregates read their states from initial_input_buffer_offset on, the Partial ones read values
        nk = 1 if grouped else 0
        skeys = [S.col(0, I32)] if grouped else []
        child = S.scan(([I32] if grouped else []) + [I64, D38, B, F64, I64, F64, F64, F64])
        c = lambda i, t: S.col(nk + i, t)
        aggs = [S.sum_(c(1, D38), D38), S.avg(c(3, F64), F64, F64), S.variance(c(5, F64)), S.count(c(0, I64)), S.min_(c(0, I64), I64)]
        yield f"mixed/sum_avg_var_count_min/{g}", S.hash_agg(child, skeys, aggs, S.PARTIAL, expr_modes=[S.PARTIAL_MERGE] * 3 + [S.PARTIAL] * 2, initial_input_buffer_offset=nk + 1)
        child = S.scan(([I32] if grouped else []) + [I64, I64, B, I8])
        aggs = [S.first_(c(1, I64), I64), S.bit_or_agg(c(3, I8), I8), S.count(c(0, I64))]
        yield f"mixed/first_bitor_count/{g}", S.hash_agg(child, skeys, aggs, S.PARTIAL, expr_modes=[S.PARTIAL_MERGE, S.PARTIAL_MERGE, S.PARTIAL], initial_input_buffer_offset=nk + 1)


def group_key_plans():
    keyed = {"bool": B, "int8": I8, "int16": I16, "int32": I32, "int64": I64, "float32": F32, "float64": F64, "date": DATE, "timestamp": TS, "timestamp_ntz": TS_NTZ,
             "decimal_12_2": D12, "decimal_18_3": D18, "decimal_38_4": D38, "utf8": STR}
    for name, t in keyed.items():
        yield f"key/{name}", S.hash_agg(S.scan([t, I64]), [S.col(0, t)], [S.count(S.col(1, I64)), S.sum_(S.col(1, I64), I64)])
    s = S.col(0, STR)
    code = S.scalar_func("substring", [s, S.lit(1, I32), S.lit(2, I32)], STR)
    yield "key/computed_short_string", S.hash_agg(S.scan([STR, I64]), [code], [S.count(S.col(1, I64))])
    fields = [STR, I64, D38, F64, B, DATE, I32]
    cs = [S.col(i, t) for i, t in enumerate(fields)]
    yield "key/seven_keys", S.hash_agg(S.scan(fields), [code] + cs[1:] + [S.math("add", cs[6], S.lit(1, I32), I32)], [S.count(cs[1]), S.max_(cs[3], F64)])
    yield "key/two_utf8_final", S.hash_agg(S.scan([STR, STR, I64]), [S.col(0, STR), S.col(1, STR)], [S.count(S.col(2, I64))], S.FINAL)
    yield "key/no_aggregates", S.hash_agg(S.scan([I32, I64]), [S.col(0, I32), S.col(1, I64)], [])
    # below the aggregate: a Filter and a Projection that computes the key and the values
    src = S.filter_(S.scan(FIELDS), S.and_(S.gt(X, S.lit(3, I64)), S.is_not_null(F)))
    p = S.project(src, [S.math("add", K, S.lit(7, I32), I32), S.math("multiply", F, G, F64), S.check_overflow(S.math("add", DD12, DD12, S.decimal(13, 2)), S.decimal(13, 2)), X])
    aggs = [S.sum_(S.col(1, F64), F64), S.sum_(S.col(2, S.decimal(13, 2)), S.decimal(23, 2)), S.variance(S.col(1, F64)), S.first_(S.col(3, I64), I64, True)]
    yield "chain/filter_project_grouped", S.hash_agg(p, [S.col(0, I32)], aggs)
    yield "chain/filter_project_ungrouped", S.hash_agg(p, [], aggs)
    yield "chain/two_filters_grouped", S.hash_agg(S.filter_(S.filter_(S.scan(FIELDS), S.lt(F, S.lit(1.5, F64))), FLT), [K], [S.count(X), S.bit_and_agg(BY, I8)])


def refusal_plans():
    yield "refuse/nine_f64_sums", S.hash_agg(S.scan([F64] * 9), [], [S.sum_(S.col(i, F64), F64) for i in range(9)])
    yield "refuse/nine_f64_sums_grouped", S.hash_agg(S.scan([I32] + [F64] * 5), [S.col(0, I32)], [S.corr(S.col(1, F64), S.col(2, F64)), S.corr(S.col(3, F64), S.col(4, F64))])
    yield "refuse/sixty_one_keys", S.hash_agg(S.scan([I8, I64]), [S.col(0, I8)] * 61, [S.count(S.col(1, I64))])
    yield "refuse/too_many_state_columns", S.hash_agg(S.scan([I32, I64]), [S.col(0, I32)], [S.first_(S.col(1, I64), I64, i % 2 == 1) for i in range(40)])
    yield "refuse/unknown_statistics_type", S.hash_agg(S.scan([F64]), [], [S.variance(S.col(0, F64), 7)])
    yield "refuse/state_column_out_of_bound", S.hash_agg(S.scan([F64, F64]), [], [S.variance(S.col(0, F64))], S.FINAL)
    yield "refuse/project_above_aggregate", S.project(S.hash_agg(S.scan([I32, I64]), [S.col(0, I32)], [S.count(S.col(1, I64))]), [S.col(0, I32)])
    yield "refuse/ansi_integer_sum", S.hash_agg(S.scan([I64]), [], [S.sum_(S.col(0, I64), I64, S.ANSI)])


def output_plans():
    fields = [I8, I16, I32, I64, F32, F64, B, DATE, TS, D12, D38, STR]
    cs = [S.col(i, t) for i, t in enumerate(fields)]
    flt = S.gt(cs[3], S.lit(0, I64))
    for with_filter in (False, True):
        f = "filter" if with_filter else "nofilter"
        src = lambda fl=fields: S.filter_(S.scan(fl), flt) if with_filter else S.scan(fl)
        yield f"out/every_store_type/{f}", S.project(src(), cs)
        computed = [S.math("add", cs[3], S.lit(1, I64), I64), S.math("multiply", cs[5], cs[5], F64), S.is_null(cs[2]), S.cast(cs[2], I64), S.check_overflow(S.math("add", cs[9], cs[9], S.decimal(13, 2)), S.decimal(13, 2)),
                    S.lt(cs[4], S.lit(0.5, F32)), S.cast(cs[10], S.decimal(38, 6))]
        yield f"out/computed/{f}", S.project(src(), computed)
        s = cs[11]
        i = lambda v: S.lit(v, I32)
        views = [S.scalar_func("read_side_padding", [s, i(32)], STR), S.scalar_func("substring", [s, i(5), i(1000)], STR), S.scalar_func("rpad", [s, i(5), S.lit("*", STR)], STR),
                 S.scalar_func("upper", [s], STR), S.scalar_func("lower", [s], STR), s]
        yield f"out/string_views/{f}", S.project(src(), views)
        cc = lambda *a: S.scalar_func("concat", list(a), STR)
        yield f"out/concat/{f}", S.project(src(), [cc(s, S.lit("-", STR), s), cc(S.lit("id: ", STR), s), cs[2]])
        yield f"out/formatted_casts/{f}", S.project(src(), [S.cast(cs[3], STR), S.cast(cs[6], STR), S.cast(cs[9], STR), S.cast(cs[7], STR), S.cast(cs[8], STR), S.cast(cs[10], STR)])
        packed = [S.scalar_func("substring", [s, i(1), i(2)], STR), S.lit("constant", STR), S.case_when([(flt, S.lit("pos", STR))], S.lit("neg", STR))]
        yield f"out/packed_strings/{f}", S.project(src(), packed + [cs[3]])
        lfields = [I32, S.list_type(I64), S.list_type(STR), STR, S.struct_type([("a", I64, True), ("b", STR, True)])]
        k, li, ls, st, sr = [S.col(j, t) for j, t in enumerate(lfields)]
        lflt = S.gt(k, S.lit(0, I32))
        lsrc = S.filter_(S.scan(lfields), lflt) if with_filter else S.scan(lfields)
        yield f"out/nested_source/{f}", S.project(lsrc, [S.list_extract(ls, i(0)), S.list_extract(ls, i(-1), one_based=True), S.list_extract(li, i(1)), S.scalar_func("size", [li], I32),
                                                         S.get_struct_field(sr, 0), S.get_struct_field(sr, 1), st, li, sr, k])
        sp = S.scalar_func("split", [S.col(0, STR), S.lit(",", STR), S.lit(-1, I32)], S.list_type(STR, False))
        ssrc = S.filter_(S.scan([STR, I32]), S.gt(S.col(1, I32), S.lit(0, I32))) if with_filter else S.scan([STR, I32])
        yield f"out/split_elements/{f}", S.project(ssrc, [S.list_extract(sp, i(0)), S.col(0, STR), S.col(1, I32)])
    yield "out/filter_only", S.filter_(S.scan([I32, F64]), S.and_(S.gt(S.col(0, I32), S.lit(1, I32)), S.is_not_null(S.col(1, F64))))


def tpch_plans():
    yield "tpch/q1", tpch.q1_plan()
    yield "tpch/q6", tpch.q6_plan()
    for i, plan in enumerate(tpch.warm_plans()):
        leaf, chain = plan, True
        while leaf.children:
            chain = chain and len(leaf.children) == 1
            leaf = leaf.children[0]
        if chain and leaf.kind == "scan":
            yield f"tpch/warm_plan_{i}", plan
    mm = S.hash_agg(S.scan([I32, I64, F64]), [S.col(0, I32)], [S.min_(S.col(1, I64), I64), S.max_(S.col(1, I64), I64), S.min_(S.col(2, F64), F64), S.max_(S.col(2, F64), F64), S.count(S.col(1, I64))])
    yield "tpch/grouped_min_max", mm


def all_plans():
    seen = set()
    for gen in (aggregate_plans, shared_and_mixed_plans, group_key_plans, refusal_plans, output_plans, tpch_plans):
        for name, plan in gen():
            assert name not in seen, name
            seen.add(name)
            yield name, plan


def n_inputs(plan):
    leaf = plan
    while leaf.children:
        leaf = leaf.children[0]
    return len(leaf.fields)


def record(plan) -> dict:
    b = plan.encode()
    ok, text = native.check_plan(b)
    e = {"check": text if ok else "refused: " + text}
    for label, on in (("valid_off", False), ("valid_on", True)):
        try:
            d = native.plan_codegen(b, [on] * (4 * n_inputs(plan) + 8))      # (a nested source's fields and elements are columns behind the real ones)
            e[label] = hashlib.sha256(json.dumps(d, sort_keys=True).encode()).hexdigest()
        except native.CometNativeException as x:
            e[label] = "refused: " + str(x)
    return e


def corpus() -> dict:
    switches = sorted(v for v in os.environ if v.startswith("COMET_") and v != "COMET_JIT_CACHE_DIR")
    assert not switches, f"{switches} set: the corpus records what the generator makes by default"
    return {name: record(plan) for name, plan in all_plans()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    text = json.dumps(corpus(), indent=0, sort_keys=True) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
