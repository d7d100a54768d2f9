// Spark's exact percentile (Percentile: median(x), percentile(x, p), percentile_cont(p) WITHIN GROUP (ORDER BY x)) as an operator over its materialised
// child — a HashAggregate all of whose aggregate functions are percentiles, grouped or not, in Partial / PartialMerge / Final mode — and the host diagnostic
// of include/comet_amd.h over device/percentile.hpp's pick.
// Reference: native/spark-expr/src/agg_funcs/percentile.rs (wired in native/core/src/execution/planner.rs).
//
// The state of one percentile is a List<Float64>: every kept (non-NULL, not filtered out) value of the group, in no particular order, never NULL.  So the
// whole aggregate is a sort: the rows as (keys, value) are ordered by (keys ASC NULLS FIRST, value ASC NULLS LAST) with the engine's radix sort; after it a
// group is a run of rows, its kept values are the head of the run in ascending order, and
//   Partial / PartialMerge emit, per group, the run's head as the list (offsets from a scan, values by one stable compaction),
//   Final picks one or two order statistics per (group, percentage) and interpolates (device/percentile.hpp).
// PartialMerge / Final first flatten the incoming lists to (keys, value) rows, outer-style — an empty or NULL list yields one row with a NULL value, so that
// a group whose lists hold nothing keeps its row; then the same path follows.  The rows per list are counted and scanned with the Explode operator's
// kernels; the rows themselves are written by pct_flatten_kernel, one thread per OUTPUT row: Explode's own index kernel gives a list eight lanes, and the
// state of an ungrouped Partial is ONE list with every value of its partition.  Each distinct (child, FILTER) pair — each state column when merging — is sorted once, however
// many percentages read it; the sorts of different value columns leave the groups in the same order (the key bytes decide it), so their columns line up.
#include "exec_internal.hpp"
#include "device/percentile.hpp"      // (compiled for the host: comet::pct_pick as the kernel runs it)

#include "../../include/comet_amd.h"

extern "C" int comet_launch_pct_flatten(const int32_t* offs, const uint8_t* list_valid, const double* elems, const uint8_t* elem_valid, int64_t n, const int32_t* out_offs, int64_t total,
                                        uint32_t* row_idx, double* vals, uint32_t* elem_idx, uint8_t* ok, void* stream);
extern "C" int comet_launch_pct_offsets(const uint32_t* first, const int32_t* C, int64_t G, int32_t* offs, void* stream);
extern "C" int comet_launch_pct_compact(const double* vals, const uint8_t* valid_bits, const int32_t* C, int64_t n, double* out, void* stream);
extern "C" int comet_launch_pct_pick(const double* vals, const uint32_t* first, const int32_t* offs, int64_t G, const double* pcts, int nq, double* out, uint8_t* ok, void* stream);

namespace comet {

std::vector<DType> extend_struct_field_types(const std::vector<DType>& types, bool with_maps);      // exec.cpp

namespace {

constexpr size_t kPctMaxValueColumns = 4;
const char* const kUnsupported = " is not supported by the MI355X native engine";

// Structural equality of two expressions, as far as it can be told from the plan.  Telling two equal ones apart costs one more value column and gives the same
// result; calling two different ones equal would return one child's percentile for the other.  So only the node kinds below are ever equal — what Spark
// puts into a percentile's child and FILTER in practice: columns, literals, casts, comparisons and their connectives — every other kind is different from
// everything, itself included; and the fields compared are all of struct Expr's that bear on a value (plan.hpp says so there).
bool comparable_kind(ExprKind k) {
  switch (k) {
    case ExprKind::Bound: case ExprKind::Literal: case ExprKind::Cast:
    case ExprKind::Eq: case ExprKind::Neq: case ExprKind::Gt: case ExprKind::GtEq: case ExprKind::Lt: case ExprKind::LtEq: case ExprKind::EqNullSafe: case ExprKind::NeqNullSafe:
    case ExprKind::And: case ExprKind::Or: case ExprKind::Not: case ExprKind::IsNull: case ExprKind::IsNotNull: case ExprKind::In:
      return true;
    default: return false;
  }
}
}  // namespace

bool same_expr(const ExprP& a, const ExprP& b) {
  if (!a || !b) return !a && !b;
  if (!comparable_kind(a->kind) || a->kind != b->kind || a->proto_tag != b->proto_tag || a->children.size() != b->children.size()) return false;
  if (a->has_dtype != b->has_dtype || (a->has_dtype && a->dtype != b->dtype)) return false;
  if (a->eval_mode != b->eval_mode || a->fail_on_error != b->fail_on_error || a->check_divide_overflow != b->check_divide_overflow || a->one_based != b->one_based ||
      a->is_spark4_plus != b->is_spark4_plus || a->negated != b->negated || a->func != b->func || a->n_when != b->n_when || a->bound_index != b->bound_index)
    return false;
  if (a->kind == ExprKind::Literal &&
      (a->lit_null != b->lit_null || a->lit_bool != b->lit_bool || a->lit_i64 != b->lit_i64 || memcmp(&a->lit_f64, &b->lit_f64, 8) != 0 || a->lit_dec != b->lit_dec ||
       a->lit_bytes != b->lit_bytes || a->lit_case != b->lit_case || a->subquery_id != b->subquery_id))
    return false;
  for (size_t i = 0; i < a->children.size(); i++)
    if (!same_expr(a->children[i], b->children[i])) return false;
  return true;
}

namespace {

// a double the way Rust's `{}` prints it (the shortest digits that read back; "NaN", "inf")
std::string rust_display(double v) {
  if (v != v) return "NaN";
  if (std::isinf(v)) return v < 0 ? "-inf" : "inf";
  char buf[40];
  for (int prec = 1; prec <= 17; prec++) {
    snprintf(buf, sizeof buf, "%.*g", prec, v);
    if (strtod(buf, nullptr) == v) break;
  }
  return buf;
}

ExprP make_expr(ExprKind k, int tag, std::vector<ExprP> kids) {
  auto e = std::make_shared<Expr>();
  e->kind = k;
  e->proto_tag = tag;
  e->children = std::move(kids);
  return e;
}

OperatorP scan_of(const std::vector<DType>& st) {
  auto sc = std::make_shared<Operator>();
  sc->kind = OpKind::Scan;
  sc->proto_tag = 100;
  sc->scan_fields = st;
  return sc;
}

}  // namespace

bool is_percentile_agg(const Operator& op) {
  if (op.kind != OpKind::HashAgg) return false;
  for (auto& a : op.agg_exprs)
    if (a.kind == AggKind::Percentile) return true;
  return false;
}

// Everything this engine refuses about a HashAggregate that holds a percentile, by name, and what is left: the percentages and the distinct value columns
PercentileSpec percentile_spec(const Operator& op) {
  const std::string who = "percentile";
  PercentileSpec s;
  for (auto& a : op.agg_exprs)
    if (a.kind != AggKind::Percentile) {
      const char* other = agg_name(a);
      throw CometError(who + " mixed with other aggregate functions (" + (other ? other : "an unknown one") + ") in one HashAggregate" + kUnsupported);
    }
  for (int m : op.expr_modes)
    if (m != (int)op.agg_mode) throw CometError(who + " in a mixed-mode aggregate" + kUnsupported);
  if (!op.expr_modes.empty() && op.expr_modes.size() != op.agg_exprs.size())
    throw CometError("HashAggregate: expr_modes has " + std::to_string(op.expr_modes.size()) + " entries for " + std::to_string(op.agg_exprs.size()) + " aggregates");
  for (auto& a : op.agg_exprs) {
    if (a.children.size() != 1 || !a.children[0]) throw CometError(who + " expects one child");
    const ExprP& c = a.children[0];
    if ((c->kind == ExprKind::Bound || c->kind == ExprKind::Literal || c->kind == ExprKind::Cast) && c->has_dtype && c->dtype.id != TypeId::Double)
      throw CometError("SparkPercentile expects Float64 input, got " + c->dtype.str() + ": " + who + " over a child that is not Float64" + kUnsupported);
    const ExprP& pe = a.percentage;
    if (!pe || pe->kind != ExprKind::Literal || pe->lit_null || !pe->has_dtype || pe->dtype.id != TypeId::Double)
      throw CometError(who + ": the percentage must be a non-NULL Float64 literal (got " +
                       (!pe ? std::string("nothing") : pe->kind != ExprKind::Literal ? std::string(expr_name(pe->proto_tag)) : pe->lit_null ? std::string("NULL") : pe->dtype.str() + " literal") +
                       "): anything else" + kUnsupported);
    const double p = pe->lit_f64;
    if (!(p >= 0.0 && p <= 1.0)) throw CometError("Percentile value must be between 0.0 and 1.0 inclusive, got " + rust_display(p) + ".");
    s.p.push_back(p);
    size_t v = 0;
    while (v < s.values.size() && !(same_expr(s.values[v].first, c) && same_expr(s.values[v].second, a.filter))) v++;
    if (v == s.values.size()) s.values.emplace_back(c, a.filter);
    s.value_of.push_back((int)v);
  }
  if (s.values.size() > kPctMaxValueColumns)
    throw CometError(who + " over more than " + std::to_string(kPctMaxValueColumns) + " distinct value columns (child, FILTER) in one HashAggregate" + kUnsupported + " (got " +
                     std::to_string(s.values.size()) + ")");
  return s;
}

// createPlan: the derived operators (see the file comment) and the types
std::vector<DType> ExecutionContext::plan_percentile(const Operator& op) {
  if (op.children.size() != 1) throw CometError("HashAggregate expects exactly one child");
  const PercentileSpec spec = percentile_spec(op);
  const std::vector<DType> st = infer_schema(*op.children[0]);
  const bool partial = op.agg_mode == AggMode::Partial;
  const size_t K = op.grouping_exprs.size(), nagg = op.agg_exprs.size();
  PercentilePlan pl;
  auto project = [&](const std::vector<ExprP>& list) {
    auto pr = std::make_shared<Operator>();
    pr->kind = OpKind::Projection;
    pr->proto_tag = 101;
    pr->children.push_back(scan_of(st));
    pr->project_list = list;
    node_id_[pr.get()] = (int)node_id_.size();
    std::vector<DType> ext = extend_struct_field_types(st, plan_->looks_into_maps);
    std::vector<bool> none(ext.size(), false);
    PipelineDesc d = generate_pipeline(*pr, none, &ext);
    if (compile_in_infer_) jit_compile(d.source);
    explain_ += d.explain;
    std::vector<DType> out;
    for (auto& c : d.out_cols) { out.push_back(c.type); out.back().virt_parent = out.back().virt_kid = -1; }
    return std::make_pair(pr, out);
  };
  DType null_double = DType::of(TypeId::Double);
  std::vector<ExprP> list = op.grouping_exprs;
  if (partial) {
    // a FILTER folds into NULL-ness: a row it rejects still counts towards its group's existence, as it does in the reference's accumulator
    for (auto& cf : spec.values) {
      if (!cf.second) { list.push_back(cf.first); continue; }
      auto nul = make_expr(ExprKind::Literal, 2, {});
      nul->dtype = null_double;
      nul->has_dtype = true;
      nul->lit_null = true;
      list.push_back(make_expr(ExprKind::If, 44, {cf.second, cf.first, nul}));
    }
  }
  std::vector<DType> pt;
  if (!list.empty()) {
    auto po = project(list);
    pt = po.second;
    if (partial) pl.proj = po.first;
    else pl.key_proj = po.first;
  }
  pl.key_types.assign(pt.begin(), pt.begin() + (long)K);
  for (size_t k = 0; k < K; k++)
    if (pl.key_types[k].is_float())
      throw CometError("percentile grouped by a " + pl.key_types[k].str() + " key" + kUnsupported + " (how -0.0 and NaN group there is a question of its own)");
  if (partial) {
    for (size_t v = 0; v < spec.values.size(); v++)
      if (pt[K + v].id != TypeId::Double) throw CometError("SparkPercentile expects Float64 input, got " + pt[K + v].str() + ": percentile over a child that is not Float64" + kUnsupported);
  } else {
    const size_t base = op.expr_modes.empty() ? K : (size_t)std::max(0, op.initial_input_buffer_offset);
    for (size_t j = 0; j < nagg; j++) {
      const size_t sc = base + j;
      if (sc >= st.size() || st[sc].id != TypeId::List || st[sc].kids.size() != 1 || st[sc].kids[0].id != TypeId::Double)
        throw CometError("percentile: the merging aggregate expects its List<Float64> state in column " + std::to_string(sc) + " of its child" +
                         (sc < st.size() ? " (got " + st[sc].str() + ")" : std::string()));
      pl.state_col.push_back((int)sc);
    }
  }
  // the sorts: by (keys ASC NULLS FIRST, value ASC NULLS LAST) over (keys, value) rows — the value under NormalizeNaNAndZero (device/percentile.hpp) —
  // and, for the group boundaries, the keys' bytes alone
  std::vector<DType> rt = pl.key_types;
  rt.push_back(DType::of(TypeId::Double));
  for (int t = 0; t < 2; t++) {
    auto so = std::make_shared<Operator>();
    so->kind = OpKind::Sort;
    so->proto_tag = 103;
    for (size_t k = 0; k < K; k++) {
      Operator::SortKey sk;
      sk.child = bound((int)k, pl.key_types[k]);
      so->sort_orders.push_back(sk);
    }
    if (t == 0) {
      Operator::SortKey sk;
      sk.child = make_expr(ExprKind::NormalizeNaNAndZero, 45, {bound((int)K, rt[K])});
      sk.nulls_last = true;
      so->sort_orders.push_back(sk);
    }
    node_id_[so.get()] = (int)node_id_.size();
    if (!so->sort_orders.empty()) {
      std::vector<bool> none(rt.size(), false);
      PipelineDesc d = generate_sort_keys(*so, rt, none);      // (refuses a key type the Sort operator does not take)
      if (compile_in_infer_) jit_compile(d.source);
    }
    (t == 0 ? pl.sort : pl.key_sort) = so;
  }
  DType list_t = DType::of(TypeId::List);
  list_t.kids.push_back(DType::of(TypeId::Double));
  list_t.kid_names.push_back("element");
  list_t.kid_nullable.push_back(1);
  pl.spec = spec;
  std::vector<DType> out = pl.key_types;
  for (size_t j = 0; j < nagg; j++) out.push_back(op.agg_mode == AggMode::Final ? DType::of(TypeId::Double) : list_t);
  explain_ += std::string("  percentile (") + (partial ? "Partial" : op.agg_mode == AggMode::Final ? "Final" : "PartialMerge") + "): " + std::to_string(nagg) + " percentile(s) over " +
              std::to_string(partial ? spec.values.size() : nagg) + (partial ? " value column(s), " : " state column(s), ") + std::to_string(K) + " grouping key(s): one sort per column\n";
  pct_plans_[&op] = pl;
  return out;
}

DevTable ExecutionContext::percentile_flatten(const DevTable& in, int sc, const DevTable& keys) {
  const DeviceColumnView& lv = in.cols.at((size_t)sc);
  if (lv.kids.size() != 1) throw CometError("percentile: the state column is not a resident list");
  if (lv.offset != 0 || lv.kids[0].offset != 0) throw CometError("percentile: a sliced (offset != 0) state column is not supported");
  const int64_t n = in.rows;
  const uint8_t* lvalid = in.has_valid[(size_t)sc] ? lv.valid : nullptr;
  const uint8_t* evalid = !lv.kid_has_valid.empty() && lv.kid_has_valid[0] ? lv.kids[0].valid : nullptr;
  DevBuf counts, tiles, out_offs;
  counts.ensure((size_t)n * 4 + 16);
  tiles.ensure((size_t)((n + 1023) / 1024 + 2) * 8);
  out_offs.ensure((size_t)(n + 1) * 4 + 16);
  if (comet_launch_explode_counts((const int32_t*)lv.data, lvalid, n, 1, (uint32_t*)counts.p, stream_) != 0) throw CometError("percentile: launch failed");
  pq_launch_u32_scan((const uint32_t*)counts.p, n, (uint64_t*)tiles.p, (int32_t*)out_offs.p, stream_);
  int32_t total = 0;
  read_small(&total, (const char*)out_offs.p + (size_t)n * 4, 4);
  if (total < 0) throw CometError("percentile: more than 2^31 kept values in one partition of the plan");
  auto row_idx = std::make_shared<DevBuf>(), vals = std::make_shared<DevBuf>(), ok = std::make_shared<DevBuf>(), bits = std::make_shared<DevBuf>();
  row_idx->ensure((size_t)total * 4 + 16);
  vals->ensure((size_t)total * 8 + 16);
  ok->ensure((size_t)total + 16);
  bits->ensure((size_t)((total + 7) / 8) + 16);
  if (comet_launch_pct_flatten((const int32_t*)lv.data, lvalid, (const double*)lv.kids[0].data, evalid, n, (const int32_t*)out_offs.p, total, (uint32_t*)row_idx->p, (double*)vals->p,
                               nullptr, (uint8_t*)ok->p, stream_) != 0)
    throw CometError("percentile: launch failed");
  if (total > 0) pq_launch_pack((const uint8_t*)ok->p, (uint8_t*)bits->p, total, stream_);
  DevTable out;
  out.rows = total;
  for (size_t c = 0; c < keys.cols.size(); c++) {
    bool hv = false;
    out.cols.push_back(take_column(keys.cols[c], keys.types[c], keys.has_valid[c], (const uint32_t*)row_idx->p, nullptr, total, hv, out.owners));
    out.types.push_back(keys.types[c]);
    out.has_valid.push_back(hv);
  }
  DeviceColumnView v;
  v.data = vals->p;
  v.valid = (const uint8_t*)bits->p;
  out.cols.push_back(v);
  out.types.push_back(DType::of(TypeId::Double));
  out.has_valid.push_back(true);
  out.owners.push_back(vals);
  out.owners.push_back(bits);
  HIP_CHECK(hipStreamSynchronize(stream_));      // counts / offsets / indices go back to their pools
  return out;
}

// The group boundaries of `sorted`, a table ordered by its grouping keys: the keys' order-preserving bytes as planes (key_sort: a Sort by the keys alone), a flag
// where a row's bytes differ from the row's before it (window_flags_kernel), the flags' scan, and first[g] = the first row of group g, first[G] = n
// (window_first_kernel).  Without keys there is one group, whatever the row count; with keys and no rows there is none.  With peer_sort — a Sort by further
// columns of the same table — fpeer[i] is 1 where row i starts a new run of equal (keys, peer key) bytes.  Shared by the percentile and the collect aggregates.
int64_t ExecutionContext::group_starts(const Operator* key_sort, const DevTable& sorted, std::shared_ptr<DevBuf>& first, const char* who, const Operator* peer_sort, DevBuf* fpeer_out) {
  const int64_t n = sorted.rows;
  const std::string name = who;
  first = std::make_shared<DevBuf>();
  if (n == 0 || (!key_sort && !peer_sort)) {
    // no keys: one group, whatever the row count (Final over no rows: one NULL; Partial: one empty list)
    first->ensure(16);
    const uint32_t fl[2] = {0, (uint32_t)n};
    write_small(first->p, fl, sizeof fl);
    return key_sort ? 0 : 1;
  }
  int Wp = 0, Wo = 0;
  std::shared_ptr<DevBuf> planes, oplanes;
  if (key_sort) planes = sort_key_planes(*key_sort, sorted, Wp);
  if (peer_sort) oplanes = sort_key_planes(*peer_sort, sorted, Wo);
  DevBuf fpart, fpeer_own, tiles, sp;
  DevBuf& fpeer = fpeer_out ? *fpeer_out : fpeer_own;
  fpart.ensure((size_t)n * 4 + 16);
  fpeer.ensure((size_t)n * 4 + 16);
  if (comet_launch_window_flags(planes ? (const uint8_t*)planes->p : nullptr, Wp, oplanes ? (const uint8_t*)oplanes->p : nullptr, Wo, n, (uint32_t*)fpart.p, (uint32_t*)fpeer.p, stream_) != 0)
    throw CometError(name + ": launch failed");
  int64_t groups = 1;
  if (!key_sort) {
    first->ensure(16);
    const uint32_t fl[2] = {0, (uint32_t)n};
    write_small(first->p, fl, sizeof fl);
  } else {
    tiles.ensure((size_t)((n + 1023) / 1024 + 2) * 8);
    sp.ensure((size_t)(n + 2) * 4);
    pq_launch_u32_scan((const uint32_t*)fpart.p, n, (uint64_t*)tiles.p, (int32_t*)sp.p, stream_);
    int32_t g32 = 0;
    read_small(&g32, (const char*)sp.p + (size_t)n * 4, 4);
    if (g32 < 1 || (int64_t)g32 > n) throw CometError("internal: " + name + ": " + std::to_string(g32) + " groups over " + std::to_string(n) + " rows");
    groups = g32;
    first->ensure((size_t)(groups + 1) * 4 + 16);
    // (the peer starts are not wanted: both outputs of window_first_kernel are fed the partition flags and their scan)
    DevBuf first_peer;
    first_peer.ensure((size_t)(groups + 1) * 4 + 16);
    if (comet_launch_window_first((const uint32_t*)fpart.p, (const int32_t*)sp.p, (const uint32_t*)fpart.p, (const int32_t*)sp.p, n, (uint32_t*)first->p, (uint32_t*)first_peer.p, stream_) != 0)
      throw CometError(name + ": launch failed");
  }
  HIP_CHECK(hipStreamSynchronize(stream_));      // planes, flags and sums go back to their pools
  return groups;
}

DevTable ExecutionContext::percentile_aggregate(const Operator& op, const DevTable& in) {
  const PercentilePlan& pl = pct_plans_.at(&op);
  const PercentileSpec& spec = pl.spec;
  const bool partial = op.agg_mode == AggMode::Partial, final_mode = op.agg_mode == AggMode::Final;
  const size_t K = pl.key_types.size(), nagg = op.agg_exprs.size();
  if (in.rows >= ((int64_t)1 << 31)) throw CometError("percentile: more than 2^31 rows in one partition of the plan");
  // ---- the value columns as (keys, value) tables ----
  std::vector<DevTable> tv;
  std::vector<int> value_of = spec.value_of;      // aggregate → its table
  if (partial) {
    DevTable t = run_chain_to_device(*pl.proj, in);
    for (size_t v = 0; v < spec.values.size(); v++) {
      DevTable s;
      s.rows = t.rows;
      s.owners = t.owners;
      for (size_t c = 0; c <= K; c++) {
        const size_t src = c < K ? c : K + v;
        s.types.push_back(t.types[src]);
        s.cols.push_back(t.cols[src]);
        s.has_valid.push_back(t.has_valid[src]);
      }
      tv.push_back(std::move(s));
    }
  } else {
    DevTable keys;
    if (pl.key_proj && in.rows > 0) keys = run_chain_to_device(*pl.key_proj, in);
    for (size_t j = 0; j < nagg; j++) {
      // state columns that are the very same buffers (a Partial's output handed over resident: its percentages over one value column share them) are flattened once
      const DeviceColumnView& a = in.cols.at((size_t)pl.state_col[j]);
      int shared = -1;
      for (size_t i = 0; i < j && shared < 0; i++) {
        const DeviceColumnView& b = in.cols[(size_t)pl.state_col[i]];
        if (a.data == b.data && a.valid == b.valid && a.offset == b.offset && a.kids.size() == 1 && b.kids.size() == 1 && a.kids[0].data == b.kids[0].data &&
            a.kids[0].valid == b.kids[0].valid && in.has_valid[(size_t)pl.state_col[j]] == in.has_valid[(size_t)pl.state_col[i]])
          shared = value_of[i];
      }
      if (shared >= 0) { value_of[j] = shared; continue; }
      value_of[j] = (int)tv.size();
      if (in.rows == 0) {
        // no state rows at all (an exhausted stream leaves columns without buffers): no (keys, value) rows either
        DevTable none;
        none.types = pl.key_types;
        none.types.push_back(DType::of(TypeId::Double));
        none.cols.assign(K + 1, DeviceColumnView());
        none.has_valid.assign(K + 1, false);
        tv.push_back(std::move(none));
        continue;
      }
      tv.push_back(percentile_flatten(in, pl.state_col[j], keys));
    }
  }
  // ---- per value column: sort, group boundaries, kept counts; then the state or the picks ----
  DevTable out;
  int64_t G = -1;
  std::vector<DeviceColumnView> agg_cols(nagg);
  std::vector<bool> agg_valid(nagg, false);
  DType list_t = DType::of(TypeId::List);
  list_t.kids.push_back(DType::of(TypeId::Double));
  list_t.kid_names.push_back("element");
  list_t.kid_nullable.push_back(1);
  for (size_t v = 0; v < tv.size(); v++) {
    const int64_t n = tv[v].rows;
    if (n >= ((int64_t)1 << 31)) throw CometError("percentile: more than 2^31 rows in one partition of the plan");
    DevTable sorted = sort_table(*pl.sort, tv[v]);
    tv[v] = DevTable();
    const DeviceColumnView& val = sorted.cols[K];
    if (n > 0 && val.offset != 0) throw CometError("internal: percentile: a sorted column with an Arrow offset");
    std::shared_ptr<DevBuf> first;
    const int64_t groups = group_starts(K ? pl.key_sort.get() : nullptr, sorted, first, "percentile");
    if (G < 0) G = groups;
    else if (G != groups) throw CometError("internal: percentile: the value columns disagree on the number of groups (" + std::to_string(G) + " and " + std::to_string(groups) + ")");
    // kept values before each row (NULLs sort last inside a group: a group's kept values are the head of its run)
    DevBuf flags, tiles, C;
    int64_t kept = n;
    const bool has_nulls = n > 0 && sorted.has_valid[K] && val.valid;
    if (has_nulls) {
      flags.ensure((size_t)n * 4 + 16);
      tiles.ensure((size_t)((n + 1023) / 1024 + 2) * 8);
      C.ensure((size_t)(n + 2) * 4);
      if (comet_launch_window_valid_flags(val.valid, n, (uint32_t*)flags.p, stream_) != 0) throw CometError("percentile: launch failed");
      pq_launch_u32_scan((const uint32_t*)flags.p, n, (uint64_t*)tiles.p, (int32_t*)C.p, stream_);
      int32_t k32 = 0;
      read_small(&k32, (const char*)C.p + (size_t)n * 4, 4);
      if (k32 < 0) throw CometError("percentile: more than 2^31 kept values in one partition of the plan");
      kept = k32;
    }
    auto offs = std::make_shared<DevBuf>();
    offs->ensure((size_t)(groups + 1) * 4 + 16);
    if (comet_launch_pct_offsets((const uint32_t*)first->p, has_nulls ? (const int32_t*)C.p : nullptr, groups, (int32_t*)offs->p, stream_) != 0) throw CometError("percentile: launch failed");
    std::shared_ptr<DevBuf> ok;      // Final: the validity bytes the pick writes and the pack reads — scratch, alive until this column's synchronise below
    if (final_mode) {
      std::vector<double> ps;
      std::vector<size_t> who;
      for (size_t j = 0; j < nagg; j++)
        if (value_of[j] == (int)v) { ps.push_back(spec.p[j]); who.push_back(j); }
      auto res = std::make_shared<DevBuf>(), bits = std::make_shared<DevBuf>();
      ok = std::make_shared<DevBuf>();
      const size_t gcap = (size_t)std::max<int64_t>(groups, 1);
      res->ensure(ps.size() * gcap * 8 + 16);
      ok->ensure(gcap + 16);
      bits->ensure((gcap + 7) / 8 + 16);
      if (comet_launch_pct_pick((const double*)val.data, (const uint32_t*)first->p, (const int32_t*)offs->p, groups, ps.data(), (int)ps.size(), (double*)res->p, (uint8_t*)ok->p, stream_) != 0)
        throw CometError("percentile: launch failed");
      if (groups > 0) pq_launch_pack((const uint8_t*)ok->p, (uint8_t*)bits->p, groups, stream_);
      for (size_t q = 0; q < who.size(); q++) {
        DeviceColumnView cv;
        cv.data = (const char*)res->p + q * (size_t)groups * 8;
        cv.valid = (const uint8_t*)bits->p;
        agg_cols[who[q]] = cv;
        agg_valid[who[q]] = true;
      }
      out.owners.push_back(res);
      out.owners.push_back(bits);
    } else {
      // the list state: offsets per group, the kept values in sorted order.  Without NULLs the sorted column is the values as it stands
      const void* values = val.data;
      if (has_nulls) {
        auto packed = std::make_shared<DevBuf>();
        packed->ensure((size_t)std::max<int64_t>(kept, 1) * 8 + 16);
        if (comet_launch_pct_compact((const double*)val.data, val.valid, (const int32_t*)C.p, n, (double*)packed->p, stream_) != 0) throw CometError("percentile: launch failed");
        values = packed->p;
        out.owners.push_back(packed);
      } else {
        for (auto& o : sorted.owners) out.owners.push_back(o);
      }
      DeviceColumnView el;
      el.data = values;
      DeviceColumnView lv;
      lv.data = offs->p;
      lv.kids.push_back(el);
      lv.kid_has_valid.push_back(0);
      lv.kid_rows = kept;
      for (size_t j = 0; j < nagg; j++)
        if (value_of[j] == (int)v) agg_cols[j] = lv;      // (each percentile its own state column; they share the buffers)
      out.owners.push_back(offs);
    }
    if (v == 0) {
      // the key columns: each group's first row
      DevTable keys;
      keys.rows = n;
      for (size_t k = 0; k < K; k++) {
        keys.types.push_back(sorted.types[k]);
        keys.cols.push_back(sorted.cols[k]);
        keys.has_valid.push_back(sorted.has_valid[k]);
      }
      DevTable kt = take_rows(keys, (const uint32_t*)first->p, 0, groups, first);      // (synchronises the stream)
      out.types = kt.types;
      out.cols = kt.cols;
      out.has_valid = kt.has_valid;
      for (auto& o : kt.owners) out.owners.push_back(o);
    }
    HIP_CHECK(hipStreamSynchronize(stream_));      // this column's scratch and its sorted table may go
  }
  out.rows = G;
  for (size_t j = 0; j < nagg; j++) {
    out.types.push_back(final_mode ? DType::of(TypeId::Double) : list_t);
    out.cols.push_back(agg_cols[j]);
    out.has_valid.push_back(agg_valid[j]);
  }
  check_device_errors();
  return out;
}

}  // namespace comet

// ---- host diagnostic (include/comet_amd.h, COMET_TEST_ABI): the pick of device/percentile.hpp, run on the host ----

extern "C" int32_t comet_spark_percentile_sorted(const double* sorted, int64_t n, double p, double* out) {
  if (!(p >= 0.0 && p <= 1.0) || n < 0 || (n > 0 && !sorted) || !out) return -1;
  if (n == 0) return 0;
  *out = comet::pct_pick(sorted, (comet::i64)n, p);
  return 1;
}
