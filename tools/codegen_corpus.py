#!/usr/bin/env python3
"""A fixed corpus of plans and what the pipeline and join generators make of each, without a GPU: per plan, the SHA-256 of the whole comet_plan_codegen JSON (kernel
source, kernels, output descriptors, fix_sums, R) with every input column's validity off and on, and comet_check_plan's text.  A refused plan is recorded with its
refusal.  tests/golden/codegen_corpus.json is this tool's output at the commit before the generator was restructured; tests/test_codegen_corpus_cpu.py compares.
That file is a record of the past and is not rewritten: plans for what the generator has learnt since go into a corpus of their own (--ansi-try-sum →
tests/golden/ansi_try_sum_codegen.json, compared by tests/test_ansi_try_sum_cpu.py; --wide-min-max → tests/golden/wide_min_max_codegen.json, compared by
tests/test_wide_min_max_agg_cpu.py), and an entry whose recorded refusal has been lifted since is RETIRED below:
it is no longer generated, its record is carried over as it stands, and the plan moves into the newer corpus under its new behaviour.

  python tools/codegen_corpus.py [--ansi-try-sum | --wide-min-max] [--out f.json]      (no COMET_* generator variable set)"""
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
        "max_d38": (lambda: S.max_(DD38, D38), [D38], False),                        # (grouped: RETIRED below)
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


def aggregate_plans(kinds=None):
    for name, (mk, state, with_filter) in (kinds if kinds is not None else aggregate_kinds()).items():
        for grouped in (False, True):
            g = "grouped" if grouped else "ungrouped"
            keys = [K] if grouped else []
            plans = [(f"agg/{name}/partial/{g}", S.hash_agg(S.scan(FIELDS), keys, [mk()]))]
            if with_filter:
                plans.append((f"agg/{name}/partial_filter/{g}", S.hash_agg(S.scan(FIELDS), keys, [filtered(mk())])))
            plans.append((f"agg/{name}/final/{g}", state_plan(mk(), state, grouped, S.FINAL)))
            plans.append((f"agg/{name}/partial_merge/{g}", state_plan(mk(), state, grouped, S.PARTIAL_MERGE)))
            for n, plan in plans:
                if kinds is not None or n not in retired():
                    yield n, plan


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


JOIN_TYPES = {"inner": S.INNER, "left_outer": S.LEFT_OUTER, "right_outer": S.RIGHT_OUTER, "full_outer": S.FULL_OUTER, "left_semi": S.LEFT_SEMI, "left_anti": S.LEFT_ANTI}
SIDES = {"build_left": S.BUILD_LEFT, "build_right": S.BUILD_RIGHT}
# the two tables every join plan reads: key, second key, one column of each key type, a Utf8 column, a payload
JL = [I64, I32, F64, D38, B, STR, I64]
JR = [I64, I32, F64, D38, B, STR, I32]


def join_plans():
    """comet_plan_codegen over a HashJoin root: the join's own kernels, probe and build fusion decided as createPlan decides them"""
    lc = [S.col(i, t) for i, t in enumerate(JL)]
    rc = [S.col(i, t) for i, t in enumerate(JR)]
    cond = S.lt(S.col(2, F64), S.col(len(JL) + 2, F64))      # bound to left ++ right
    for tn, jt in JOIN_TYPES.items():
        for sn, side in SIDES.items():
            yield f"join/type/{tn}/{sn}", S.hash_join(S.scan(JL), S.scan(JR), [lc[0]], [rc[0]], jt, side)
            yield f"join/type/{tn}/{sn}/cond", S.hash_join(S.scan(JL), S.scan(JR), [lc[0]], [rc[0]], jt, side, cond)
    short = lambda c: S.scalar_func("substring", [c, S.lit(1, I32), S.lit(2, I32)], STR)
    keys = {"int32_int64": ([lc[1], lc[0]], [rc[1], rc[0]]), "float64": ([lc[2]], [rc[2]]), "decimal_38": ([lc[3]], [rc[3]]), "bool": ([lc[4]], [rc[4]]),
            "computed_short_string": ([short(lc[5])], [short(rc[5])])}
    for kn, (lk, rk) in keys.items():
        for tn in ("inner", "left_semi"):
            for sn, side in SIDES.items():
                yield f"join/key/{kn}/{tn}/{sn}", S.hash_join(S.scan(JL), S.scan(JR), lk, rk, JOIN_TYPES[tn], side)
    # fusion: a chain with a Filter and a computed key fuses into the probe kernel, a chain whose Filters are isnotnull only into the build passes
    def probe_chain(fields):
        c = [S.col(i, t) for i, t in enumerate(fields)]
        src = S.filter_(S.scan(fields), S.and_(S.is_not_null(c[0]), S.gt(c[6], S.lit(3, fields[6]))))
        return S.project(src, [S.math("add", c[0], S.lit(1, I64), I64), c[2], c[5], c[6]]), [I64, F64, STR, fields[6]]

    def build_chain(fields):
        c = [S.col(i, t) for i, t in enumerate(fields)]
        return S.project(S.filter_(S.scan(fields), S.is_not_null(c[0])), [c[0], c[2], c[5], c[6]]), [I64, F64, STR, fields[6]]

    for fn in ("none", "probe", "build", "both"):
        for tn in ("inner", "left_outer", "full_outer", "left_semi", "left_anti"):
            for sn, side in SIDES.items():
                for with_cond in (False, True):
                    sides = []
                    for is_left, fields in ((True, JL), (False, JR)):
                        is_build = is_left == (side == S.BUILD_LEFT)
                        if fn == "both" or fn == ("build" if is_build else "probe"):
                            sides.append(build_chain(fields) if is_build else probe_chain(fields))
                        else:
                            sides.append((S.scan(fields), fields))
                    (l, lt_), (r, rt_) = sides
                    if fn == "none" and not with_cond:
                        continue      # (join/type/… above)
                    c = S.lt(S.col(lt_.index(F64), F64), S.col(len(lt_) + rt_.index(F64), F64)) if with_cond else None
                    yield f"join/fused_{fn}/{tn}/{sn}" + ("/cond" if with_cond else ""), S.hash_join(l, r, [S.col(0, I64)], [S.col(0, I64)], JOIN_TYPES[tn], side, c)
    # a Utf8 payload column on one side only (gathered after the emit)
    for sn, side in SIDES.items():
        yield f"join/utf8_payload/left/{sn}", S.hash_join(S.scan([I64, STR]), S.scan([I64, F64]), [S.col(0, I64)], [S.col(0, I64)], S.LEFT_OUTER, side)
        yield f"join/utf8_payload/right/{sn}", S.hash_join(S.scan([I64, F64]), S.scan([I64, STR]), [S.col(0, I64)], [S.col(0, I64)], S.LEFT_OUTER, side)
    # (the root is the Projection: comet_check_plan's text is what this entry pins)
    yield "join/outer_under_projection", S.project(S.hash_join(S.scan(JL), S.scan(JR), [lc[0]], [rc[0]], S.FULL_OUTER, S.BUILD_RIGHT),
                                                     [S.col(0, I64), S.math("add", S.col(6, I64), S.cast(S.col(len(JL) + 6, I32), I64), I64)])
    # refusals
    na = S.hash_join(S.scan(JL), S.scan(JR), [lc[0]], [rc[0]], S.LEFT_ANTI, S.BUILD_RIGHT)
    na.null_aware_anti = True
    yield "join/refuse/null_aware_anti", na
    yield "join/refuse/key_types_differ", S.hash_join(S.scan(JL), S.scan(JR), [lc[0]], [rc[3]], S.INNER, S.BUILD_RIGHT)
    yield "join/refuse/key_counts_differ", S.hash_join(S.scan(JL), S.scan(JR), [lc[0], lc[1]], [rc[0]], S.INNER, S.BUILD_RIGHT)
    yield "join/refuse/too_many_output_columns", S.hash_join(S.scan([I64] * 11), S.scan([I64] * 11), [S.col(0, I64)], [S.col(0, I64)], S.INNER, S.BUILD_RIGHT)
    yield "join/refuse/too_many_input_columns", S.hash_join(S.scan([I64] * 13), S.scan([I64] * 12), [S.col(0, I64)], [S.col(0, I64)], S.LEFT_SEMI, S.BUILD_RIGHT)
    # (the fused functor refuses a computed Utf8 column; the join then runs over the materialised chain)
    pc = S.project(S.filter_(S.scan(JL), S.gt(lc[6], S.lit(3, I64))), [lc[0], short(lc[5])])
    yield "join/refuse/computed_utf8_under_fused_probe", S.hash_join(pc, S.scan(JR), [S.col(0, I64)], [rc[0]], S.INNER, S.BUILD_RIGHT)


# entries of tests/golden/codegen_corpus.json whose refusal has been lifted: name → (what was recorded, where the plan is held now)
RETIRED = {
    "refuse/ansi_integer_sum": ("refused: ANSI/TRY integer sum is not supported in the GPU pipeline yet", "ansi_try_sum_plans: lifted/ansi_integer_sum"),
}
# (a table of its own: tests/test_ansi_try_sum_cpu.py pins RETIRED to the entry its pull request retired; retired() is both)
WIDE_MIN_MAX_REFUSAL = "refused: min/max of a decimal wider than 18 digits is not supported in a grouped GPU aggregate yet"
RETIRED_WIDE_MIN_MAX = {
    "agg/max_d38/partial/grouped": (WIDE_MIN_MAX_REFUSAL, "wide_min_max_plans: agg/max_d38/partial/grouped"),
    "agg/max_d38/partial_merge/grouped": (WIDE_MIN_MAX_REFUSAL, "wide_min_max_plans: agg/max_d38/partial_merge/grouped"),
    "agg/max_d38/final/grouped": (WIDE_MIN_MAX_REFUSAL, "wide_min_max_plans: agg/max_d38/final/grouped"),
}


def retired() -> dict:
    return {**RETIRED, **RETIRED_WIDE_MIN_MAX}


def ansi_try_sum_plans():
    """ANSI / TRY integer sums in every mode, grouped and not, and unscaled_value / make_decimal: the corpus of tests/golden/ansi_try_sum_codegen.json"""
    kinds = {
        "sum_i8_ansi": (lambda: S.sum_(BY, I64, S.ANSI), [I64], False),              # proven by the input's bound: LEGACY's words
        "sum_i32_ansi": (lambda: S.sum_(XI, I64, S.ANSI), [I64], False),             # dynamic: the positive and the negative sum
        "sum_i64_ansi": (lambda: S.sum_(X, I64, S.ANSI), [I64], True),
        "sum_i16_try": (lambda: S.sum_(SH, I64, S.TRY), [I64, B], False),
        "sum_i64_try": (lambda: S.sum_(X, I64, S.TRY), [I64, B], True),
        "sum_unscaled_d12_ansi": (lambda: S.sum_(S.unscaled_value(DD12), I64, S.ANSI), [I64], False),
    }
    yield from aggregate_plans(kinds)
    yield "lifted/ansi_integer_sum", S.hash_agg(S.scan([I64]), [], [S.sum_(S.col(0, I64), I64, S.ANSI)])      # (RETIRED["refuse/ansi_integer_sum"])
    for grouped in (False, True):
        g = "grouped" if grouped else "ungrouped"
        keys = [K] if grouped else []
        yield f"shared/legacy_ansi_try_same_value/{g}", S.hash_agg(S.scan(FIELDS), keys, [S.sum_(X, I64), S.sum_(X, I64, S.ANSI), S.sum_(X, I64, S.TRY), S.count(X)])
        nk = 1 if grouped else 0
        child = S.scan([I32] * nk + [I64, I64, B, I64])
        c = lambda i, t: S.col(nk + i, t)
        aggs = [S.sum_(c(0, I64), I64, S.TRY), S.sum_(c(0, I64), I64, S.ANSI), S.count(c(0, I64))]
        yield f"mixed/try_ansi_count/{g}", S.hash_agg(child, [S.col(0, I32)] * nk, aggs, S.PARTIAL, expr_modes=[S.PARTIAL_MERGE, S.PARTIAL_MERGE, S.PARTIAL], initial_input_buffer_offset=nk + 1)
    scan = S.scan([D12, I64])
    yield "out/unscaled_value_make_decimal", S.project(scan, [S.unscaled_value(S.col(0, D12)), S.make_decimal(S.col(1, I64), 17, 2), S.make_decimal(S.col(1, I64), 17, 2, null_on_overflow=False),
                                                             S.make_decimal(S.unscaled_value(S.col(0, D12)), 22, 2, null_on_overflow=False)])
    yield "refuse/unscaled_value_of_a_wide_decimal", S.hash_agg(S.scan([D38]), [], [S.sum_(S.unscaled_value(S.col(0, D38)), I64, S.ANSI)])
    yield "refuse/make_decimal_of_an_int", S.project(S.scan([I32]), [S.make_decimal(S.col(0, I32), 17, 2)])
    yield "refuse/final_try_sum_without_its_flag", S.hash_agg(S.scan([I64, I64]), [], [S.sum_(S.col(0, I64), I64, S.TRY)], S.FINAL)


def wide_min_max_plans():
    """grouped min / max of a decimal wider than 18 digits in every mode (the three RETIRED plans and a min twin), beside other aggregates, and the cast of a narrow
    decimal whose bound keeps it on the one-word min / max: the corpus of tests/golden/wide_min_max_codegen.json"""
    kinds = {
        "max_d38": (lambda: S.max_(DD38, D38), [D38], True),
        "min_d38": (lambda: S.min_(DD38, D38), [D38], True),
    }
    for name, plan in aggregate_plans(kinds):
        if name.endswith("/grouped"):
            yield name, plan
    yield "mixed/max_d38_first_sum_count/grouped", S.hash_agg(S.scan(FIELDS), [K], [S.max_(DD38, D38), S.first_(X, I64), S.sum_(DD38, D38), S.count(DD38), S.min_(DD38, D38)])
    yield "shortcut/max_cast_d12_as_d22/grouped", S.hash_agg(S.scan(FIELDS), [K], [S.max_(S.cast(DD12, D22), D22)])


def all_plans():
    seen = set()
    for gen in (aggregate_plans, shared_and_mixed_plans, group_key_plans, refusal_plans, output_plans, tpch_plans, join_plans):
        for name, plan in gen():
            assert name not in seen, name
            seen.add(name)
            yield name, plan


def n_inputs(plan):
    """the columns of every Scan leaf (a join's has_valid covers the left source, then the right source)"""
    return len(plan.fields) if not plan.children else sum(n_inputs(c) for c in plan.children)


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
    out = {name: record(plan) for name, plan in all_plans()}
    for name, (recorded, _) in retired().items():
        assert name not in out, name
        out[name] = {"check": recorded, "valid_off": recorded, "valid_on": recorded}
    return out


def ansi_try_sum_corpus() -> dict:
    return {name: record(plan) for name, plan in ansi_try_sum_plans()}


def wide_min_max_corpus() -> dict:
    return {name: record(plan) for name, plan in wide_min_max_plans()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--ansi-try-sum", action="store_true", help="the corpus of tests/golden/ansi_try_sum_codegen.json instead")
    ap.add_argument("--wide-min-max", action="store_true", help="the corpus of tests/golden/wide_min_max_codegen.json instead")
    a = ap.parse_args()
    made = ansi_try_sum_corpus() if a.ansi_try_sum else wide_min_max_corpus() if a.wide_min_max else corpus()
    text = json.dumps(made, indent=0, sort_keys=True) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
