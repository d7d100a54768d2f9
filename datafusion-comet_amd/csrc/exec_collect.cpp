// collect_list / array_agg and collect_set as an operator over the materialised child — a HashAggregate all of whose aggregate functions are collects, grouped
// or not, in Partial / PartialMerge / Final mode, any mix of the two functions.
// Reference: native/core/src/execution/planner.rs (AggExprStruct::CollectList / CollectSet), spark/src/main/scala/org/apache/comet/serde/aggregates.scala.
//
// State and result are the same thing, a List<element> (element field nullable) that never is NULL and never holds a NULL: every kept (non-NULL, not filtered
// out) value of the group — so PartialMerge and Final are one computation.  The aggregate never looks at a value; it works on row numbers:
//   the rows as (keys, value) are sorted with the engine's radix sort — collect_list by the keys alone (the sort is stable, so a group's values keep the order
//   they arrived in: batches in the order pulled, rows in batch order; without keys there is no sort at all), collect_set by (keys ASC NULLS FIRST, value ASC
//   NULLS LAST), which puts equal values next to each other;
//   a group is then a run of rows (group_starts, shared with the percentile aggregate), and a row is kept when its value is not NULL and — for a set — it is the
//   first of its run of equal (group, value) key bytes (window_flags_kernel's peer flag over the value's own order-preserving bytes);
//   the kept flags' scan gives each group's offset (pct_offsets_kernel) and each kept row's slot (collect_index_kernel); the elements are one take_column of the
//   sorted value column by those row numbers — any type, Utf8 and 128-bit decimals included.
// A set's elements therefore stand in ascending order of the engine's sort key, a list's in arrival order; both are the same bits for every batch size.
// A FILTER (Partial only) is evaluated as a Boolean column beside the value and folded into the value's validity bits (collect_mask_kernel): a rejected row
// is a NULL value, which still makes its group exist.  (Not as If(filter, child, NULL) the way the percentile does it for its doubles: a computed Utf8 value of
// the generated pipelines holds at most 15 bytes.)
// PartialMerge / Final flatten each incoming state column to (parent row, element index) rows with the percentile's pct_flatten_kernel, outer-style — an empty
// or NULL list yields one row with a NULL value, so its group survives —, take the keys by parent row and the element by element index, and go on as above:
// state rows in input order, each list's elements in list order.
#include "exec_internal.hpp"

extern "C" int comet_launch_pct_flatten(const int32_t* offs, const uint8_t* list_valid, const double* elems, const uint8_t* elem_valid, int64_t n, const int32_t* out_offs, int64_t total,
                                        uint32_t* row_idx, double* vals, uint32_t* elem_idx, uint8_t* ok, void* stream);
extern "C" int comet_launch_pct_offsets(const uint32_t* first, const int32_t* C, int64_t G, int32_t* offs, void* stream);
extern "C" int comet_launch_collect_mask(const uint8_t* valid, const uint8_t* fvalid, const uint8_t* fdata, int64_t n, uint8_t* out, void* stream);
extern "C" int comet_launch_collect_keep(const uint8_t* valid, const uint32_t* fpeer, int64_t n, uint32_t* keep, void* stream);
extern "C" int comet_launch_collect_index(const uint32_t* keep, const int32_t* C, int64_t n, uint32_t* idx, void* stream);

namespace comet {

std::vector<DType> extend_struct_field_types(const std::vector<DType>& types, bool with_maps);      // exec.cpp

namespace {

constexpr size_t kCollectMaxValueColumns = 4;
const char* const kUnsupported = " is not supported by the MI355X native engine";

bool is_collect(const AggExpr& a) { return a.kind == AggKind::CollectList || a.kind == AggKind::CollectSet; }

// what a collect's element may be: refuses the rest by name
void check_element(const std::string& who, bool set, const DType& t) {
  switch (t.id) {
    case TypeId::Bool: case TypeId::Int8: case TypeId::Int16: case TypeId::Int32: case TypeId::Int64: case TypeId::Date: case TypeId::Timestamp: case TypeId::TimestampNtz:
    case TypeId::Decimal: case TypeId::String:
      return;
    case TypeId::Float: case TypeId::Double:
      if (set)
        throw CometError(who + " over a " + t.str() + " child" + kUnsupported +
                         " (whether the reference's set keeps -0.0 beside 0.0 and one NaN payload beside another cannot be told from its planner; collect_list copies floats bit for bit)");
      return;
    case TypeId::Bytes: throw CometError(who + " over a Binary child" + kUnsupported);
    case TypeId::Struct: case TypeId::List: case TypeId::Map: throw CometError(who + " over a nested (" + t.str() + ") child" + kUnsupported);
    default: throw CometError(who + " over a " + t.str() + " child" + kUnsupported);
  }
}

DType list_of(const DType& elem) {
  DType l = DType::of(TypeId::List);
  l.kids.push_back(elem);
  l.kids.back().virt_parent = l.kids.back().virt_kid = -1;
  l.kid_names.push_back("element");
  l.kid_nullable.push_back(1);
  return l;
}

}  // namespace

bool is_collect_agg(const Operator& op) {
  if (op.kind != OpKind::HashAgg) return false;
  for (auto& a : op.agg_exprs)
    if (is_collect(a)) return true;
  return false;
}

// Everything this engine refuses about a HashAggregate that holds a collect, by name, and what is left: the distinct value columns
CollectSpec collect_spec(const Operator& op) {
  std::string who = "collect_list";
  for (auto& a : op.agg_exprs)
    if (is_collect(a)) { who = agg_name(a); break; }
  CollectSpec s;
  for (auto& a : op.agg_exprs)
    if (!is_collect(a)) {
      const char* other = agg_name(a);
      throw CometError(who + " mixed with other aggregate functions (" + (other ? other : "an unknown one") + ") in one HashAggregate" + kUnsupported);
    }
  for (int m : op.expr_modes)
    if (m != (int)op.agg_mode) throw CometError(who + " in a mixed-mode aggregate" + kUnsupported);
  if (!op.expr_modes.empty() && op.expr_modes.size() != op.agg_exprs.size())
    throw CometError("HashAggregate: expr_modes has " + std::to_string(op.expr_modes.size()) + " entries for " + std::to_string(op.agg_exprs.size()) + " aggregates");
  for (auto& a : op.agg_exprs) {
    const std::string me = agg_name(a);
    if (a.children.size() != 1 || !a.children[0]) throw CometError(me + " expects one child");
    if (a.dtype.id != TypeId::List || a.dtype.kids.size() != 1)
      throw CometError(me + ": the aggregate's datatype must be the List of its element type (got " + a.dtype.str() + ")");
    CollectSpec::Value val;
    val.child = a.children[0];
    val.filter = a.filter;
    val.set = a.kind == AggKind::CollectSet;
    val.elem = a.dtype.kids[0];
    check_element(me, val.set, val.elem);
    size_t v = 0;
    while (v < s.values.size() && !(s.values[v].set == val.set && same_expr(s.values[v].child, val.child) && same_expr(s.values[v].filter, val.filter))) v++;
    if (v == s.values.size()) s.values.push_back(val);
    s.value_of.push_back((int)v);
  }
  if (s.values.size() > kCollectMaxValueColumns)
    throw CometError(who + " over more than " + std::to_string(kCollectMaxValueColumns) + " distinct value columns (function, child, FILTER) in one HashAggregate" + kUnsupported + " (got " +
                     std::to_string(s.values.size()) + ")");
  return s;
}

// createPlan: the derived operators (see the file comment) and the types
std::vector<DType> ExecutionContext::plan_collect(const Operator& op) {
  if (op.children.size() != 1) throw CometError("HashAggregate expects exactly one child");
  const CollectSpec spec = collect_spec(op);
  const std::vector<DType> st = infer_schema(*op.children[0]);
  const bool partial = op.agg_mode == AggMode::Partial;
  const size_t K = op.grouping_exprs.size(), nagg = op.agg_exprs.size();
  CollectPlan pl;
  std::vector<ExprP> list = op.grouping_exprs;
  if (partial) {
    for (auto& val : spec.values) {
      pl.val_col.push_back((int)list.size());
      list.push_back(val.child);
      pl.flt_col.push_back(val.filter ? (int)list.size() : -1);
      if (val.filter) list.push_back(val.filter);
    }
  }
  std::vector<DType> pt;
  if (!list.empty()) {
    auto pr = std::make_shared<Operator>();
    pr->kind = OpKind::Projection;
    pr->proto_tag = 101;
    auto sc = std::make_shared<Operator>();
    sc->kind = OpKind::Scan;
    sc->proto_tag = 100;
    sc->scan_fields = st;
    pr->children.push_back(sc);
    pr->project_list = list;
    node_id_[pr.get()] = (int)node_id_.size();
    std::vector<DType> ext = extend_struct_field_types(st, plan_->looks_into_maps);
    std::vector<bool> none(ext.size(), false);
    PipelineDesc d = generate_pipeline(*pr, none, &ext);
    if (compile_in_infer_) jit_compile(d.source);
    explain_ += d.explain;
    for (auto& c : d.out_cols) { pt.push_back(c.type); pt.back().virt_parent = pt.back().virt_kid = -1; }
    (partial ? pl.proj : pl.key_proj) = pr;
  }
  pl.key_types.assign(pt.begin(), pt.begin() + (long)K);
  for (size_t k = 0; k < K; k++)
    if (pl.key_types[k].is_float())
      throw CometError("collect_list / collect_set grouped by a " + pl.key_types[k].str() + " key" + kUnsupported + " (how -0.0 and NaN group there is a question of its own)");
  std::vector<bool> is_set;
  if (partial) {
    for (size_t v = 0; v < spec.values.size(); v++) {
      const std::string me = spec.values[v].set ? "collect_set" : "collect_list";
      const DType& ct = pt[(size_t)pl.val_col[v]];
      check_element(me, spec.values[v].set, ct);
      if (ct != spec.values[v].elem)
        throw CometError(me + ": the child is " + ct.str() + " but the aggregate's datatype says List<" + spec.values[v].elem.str() + ">");
      if (pl.flt_col[v] >= 0 && pt[(size_t)pl.flt_col[v]].id != TypeId::Bool) throw CometError(me + ": the FILTER is " + pt[(size_t)pl.flt_col[v]].str() + ", not Boolean");
      pl.elem_types.push_back(ct);
      is_set.push_back(spec.values[v].set);
    }
  } else {
    const size_t base = op.expr_modes.empty() ? K : (size_t)std::max(0, op.initial_input_buffer_offset);
    for (size_t j = 0; j < nagg; j++) {
      const CollectSpec::Value& val = spec.values[(size_t)spec.value_of[j]];
      const std::string me = val.set ? "collect_set" : "collect_list";
      const size_t sc = base + j;
      if (sc >= st.size() || st[sc].id != TypeId::List || st[sc].kids.size() != 1 || st[sc].kids[0] != val.elem)
        throw CometError(me + ": the merging aggregate expects its List<" + val.elem.str() + "> state in column " + std::to_string(sc) + " of its child" +
                         (sc < st.size() ? " (got " + st[sc].str() + ")" : std::string()));
      pl.state_col.push_back((int)sc);
      pl.elem_types.push_back(val.elem);
      is_set.push_back(val.set);
    }
  }
  // per value column its sorts over (keys, value) rows; each is generated here, which refuses a key type the Sort operator does not take
  for (size_t c = 0; c < pl.elem_types.size(); c++) {
    std::vector<DType> rt = pl.key_types;
    rt.push_back(pl.elem_types[c]);
    for (int t = 0; t < 3; t++) {      // 0: the sort, 1: the keys alone, 2: the value alone
      auto so = std::make_shared<Operator>();
      so->kind = OpKind::Sort;
      so->proto_tag = 103;
      if (t != 2)
        for (size_t k = 0; k < K; k++) {
          Operator::SortKey sk;
          sk.child = bound((int)k, pl.key_types[k]);
          so->sort_orders.push_back(sk);
        }
      if (t == 2 || (t == 0 && is_set[c])) {
        Operator::SortKey sk;
        sk.child = bound((int)K, rt[K]);
        sk.nulls_last = true;
        so->sort_orders.push_back(sk);
      }
      if (so->sort_orders.empty() || (t == 2 && !is_set[c])) so = nullptr;
      if (so) {
        node_id_[so.get()] = (int)node_id_.size();
        std::vector<bool> none(rt.size(), false);
        PipelineDesc d = generate_sort_keys(*so, rt, none);
        if (compile_in_infer_) jit_compile(d.source);
      }
      (t == 0 ? pl.sort : t == 1 ? pl.key_sort : pl.val_sort).push_back(so);
    }
  }
  pl.spec = spec;
  std::vector<DType> out = pl.key_types;
  for (size_t j = 0; j < nagg; j++) out.push_back(list_of(spec.values[(size_t)spec.value_of[j]].elem));
  size_t nset = 0;
  for (bool b : is_set) nset += b;
  explain_ += std::string("  collect (") + (partial ? "Partial" : op.agg_mode == AggMode::Final ? "Final" : "PartialMerge") + "): " + std::to_string(nagg) + " collect(s) over " +
              std::to_string(is_set.size() - nset) + " list and " + std::to_string(nset) + " set " + (partial ? "value column(s), " : "state column(s), ") + std::to_string(K) +
              " grouping key(s): one sort per column\n";
  collect_plans_[&op] = pl;
  return out;
}

DevTable ExecutionContext::collect_flatten(const DevTable& in, int sc, const DType& elem, const DevTable& keys) {
  const DeviceColumnView& lv = in.cols.at((size_t)sc);
  if (lv.kids.size() != 1) throw CometError("collect: the state column is not a resident list");
  if (lv.offset != 0 || lv.kids[0].offset != 0) throw CometError("collect: a sliced (offset != 0) state column is not supported");
  const int64_t n = in.rows;
  const uint8_t* lvalid = in.has_valid[(size_t)sc] ? lv.valid : nullptr;
  const uint8_t* evalid = !lv.kid_has_valid.empty() && lv.kid_has_valid[0] ? lv.kids[0].valid : nullptr;
  DevBuf counts, tiles, out_offs;
  counts.ensure((size_t)n * 4 + 16);
  tiles.ensure((size_t)((n + 1023) / 1024 + 2) * 8);
  out_offs.ensure((size_t)(n + 1) * 4 + 16);
  if (comet_launch_explode_counts((const int32_t*)lv.data, lvalid, n, 1, (uint32_t*)counts.p, stream_) != 0) throw CometError("collect: launch failed");
  pq_launch_u32_scan((const uint32_t*)counts.p, n, (uint64_t*)tiles.p, (int32_t*)out_offs.p, stream_);
  int32_t total = 0, elements = 0;
  read_small(&total, (const char*)out_offs.p + (size_t)n * 4, 4);
  if (total < 0) throw CometError("collect: more than 2^31 elements in one partition of the plan");
  read_small(&elements, (const char*)lv.data + (size_t)n * 4, 4);      // the lists' last offset: how far into the element column they reach
  auto row_idx = std::make_shared<DevBuf>(), elem_idx = std::make_shared<DevBuf>(), ok = std::make_shared<DevBuf>(), bits = std::make_shared<DevBuf>();
  row_idx->ensure((size_t)total * 4 + 16);
  elem_idx->ensure((size_t)total * 4 + 16);
  ok->ensure((size_t)total + 16);
  bits->ensure((size_t)((total + 7) / 8) + 16);
  if (comet_launch_pct_flatten((const int32_t*)lv.data, lvalid, nullptr, evalid, n, (const int32_t*)out_offs.p, total, (uint32_t*)row_idx->p, nullptr, (uint32_t*)elem_idx->p,
                               (uint8_t*)ok->p, stream_) != 0)
    throw CometError("collect: launch failed");
  if (total > 0) pq_launch_pack((const uint8_t*)ok->p, (uint8_t*)bits->p, total, stream_);
  DevTable out;
  out.rows = total;
  for (size_t c = 0; c < keys.cols.size(); c++) {
    bool hv = false;
    out.cols.push_back(take_column(keys.cols[c], keys.types[c], keys.has_valid[c], (const uint32_t*)row_idx->p, nullptr, total, hv, out.owners));
    out.types.push_back(keys.types[c]);
    out.has_valid.push_back(hv);
  }
  DeviceColumnView ev;
  if (elements > 0) {
    // the element by its index, whatever its type (as Explode takes it); a row without a kept element reads element 0 and is masked out
    bool hv_unused = false;
    ev = take_column(lv.kids[0], elem, false, (const uint32_t*)elem_idx->p, (const uint8_t*)ok->p, total, hv_unused, out.owners);
  } else {
    // not one element in any list: every row is a NULL value — zeroed buffers of the element's layout (all-zero offsets for Utf8)
    const bool is_str = elem.id == TypeId::String;
    const size_t bytes = is_str ? (size_t)(total + 1) * 4 : elem.id == TypeId::Bool ? (size_t)((total + 7) / 8) : (size_t)total * (size_t)fixed_width(elem);
    auto data = std::make_shared<DevBuf>();
    data->ensure(bytes + 16);
    HIP_CHECK(hipMemsetAsync(data->p, 0, bytes + 16, stream_));
    ev.data = data->p;
    out.owners.push_back(data);
    if (is_str) {
      auto aux = std::make_shared<DevBuf>();
      aux->ensure(16);
      ev.aux = aux->p;
      out.owners.push_back(aux);
    }
  }
  ev.valid = (const uint8_t*)bits->p;
  out.cols.push_back(ev);
  out.types.push_back(elem);
  out.has_valid.push_back(true);
  out.owners.push_back(bits);
  HIP_CHECK(hipStreamSynchronize(stream_));      // counts / offsets / indices / ok bytes go back to their pools
  return out;
}

DevTable ExecutionContext::collect_aggregate(const Operator& op, const DevTable& in) {
  const CollectPlan& pl = collect_plans_.at(&op);
  const CollectSpec& spec = pl.spec;
  const bool partial = op.agg_mode == AggMode::Partial;
  const size_t K = pl.key_types.size(), nagg = op.agg_exprs.size(), ncol = pl.elem_types.size();
  if (in.rows >= ((int64_t)1 << 31)) throw CometError("collect: more than 2^31 rows in one partition of the plan");
  // ---- the value columns as (keys, value) tables ----
  std::vector<DevTable> tv;
  std::vector<bool> is_set;
  std::vector<int> value_of;      // aggregate → its table
  if (partial) {
    value_of = spec.value_of;
    DevTable t = run_chain_to_device(*pl.proj, in);
    for (size_t v = 0; v < ncol; v++) {
      DevTable s;
      s.rows = t.rows;
      s.owners = t.owners;
      for (size_t c = 0; c <= K; c++) {
        const size_t src = c < K ? c : (size_t)pl.val_col[v];
        s.types.push_back(t.types[src]);
        s.cols.push_back(t.cols[src]);
        s.has_valid.push_back(t.has_valid[src]);
      }
      if (pl.flt_col[v] >= 0 && t.rows > 0) {
        // the FILTER folds into NULL-ness: a row it rejects (FALSE or NULL) still counts towards its group's existence
        const size_t f = (size_t)pl.flt_col[v];
        if (s.cols[K].offset != 0 || t.cols[f].offset != 0) throw CometError("internal: collect: a projected column with an Arrow offset");
        auto mask = std::make_shared<DevBuf>();
        mask->ensure((size_t)((t.rows + 7) / 8) + 16);
        if (comet_launch_collect_mask(s.has_valid[K] ? s.cols[K].valid : nullptr, t.has_valid[f] ? t.cols[f].valid : nullptr, (const uint8_t*)t.cols[f].data, t.rows, (uint8_t*)mask->p,
                                      stream_) != 0)
          throw CometError("collect: launch failed");
        s.cols[K].valid = (const uint8_t*)mask->p;
        s.has_valid[K] = true;
        s.owners.push_back(mask);
      }
      is_set.push_back(spec.values[v].set);
      tv.push_back(std::move(s));
    }
  } else {
    DevTable keys;
    if (pl.key_proj && in.rows > 0) keys = run_chain_to_device(*pl.key_proj, in);
    for (size_t j = 0; j < nagg; j++) {
      value_of.push_back((int)j);
      is_set.push_back(spec.values[(size_t)spec.value_of[j]].set);
      if (in.rows == 0) {
        // no state rows at all (an exhausted stream leaves columns without buffers): no (keys, value) rows either
        DevTable none;
        none.types = pl.key_types;
        none.types.push_back(pl.elem_types[j]);
        none.cols.assign(K + 1, DeviceColumnView());
        none.has_valid.assign(K + 1, false);
        tv.push_back(std::move(none));
        continue;
      }
      tv.push_back(collect_flatten(in, pl.state_col[j], pl.elem_types[j], keys));
    }
  }
  // ---- per value column: sort, group boundaries, kept rows; then the list ----
  DevTable out;
  int64_t G = -1;
  std::vector<DeviceColumnView> agg_cols(nagg);
  for (size_t v = 0; v < tv.size(); v++) {
    const int64_t n = tv[v].rows;
    if (n >= ((int64_t)1 << 31)) throw CometError("collect: more than 2^31 rows in one partition of the plan");
    const bool set = is_set[v];
    // (a list without keys needs no sort: its rows stand in arrival order already)
    DevTable sorted = pl.sort[v] && n > 0 ? sort_table(*pl.sort[v], tv[v]) : std::move(tv[v]);
    tv[v] = DevTable();
    const DeviceColumnView& val = sorted.cols[K];
    if (n > 0 && val.offset != 0) throw CometError("internal: collect: a value column with an Arrow offset");
    std::shared_ptr<DevBuf> first;
    DevBuf fpeer;
    const int64_t groups = group_starts(K ? pl.key_sort[v].get() : nullptr, sorted, first, "collect", set ? pl.val_sort[v].get() : nullptr, set ? &fpeer : nullptr);
    if (G < 0) G = groups;
    else if (G != groups) throw CometError("internal: collect: the value columns disagree on the number of groups (" + std::to_string(G) + " and " + std::to_string(groups) + ")");
    const bool has_nulls = n > 0 && sorted.has_valid[K] && val.valid;
    auto offs = std::make_shared<DevBuf>();
    offs->ensure((size_t)(groups + 1) * 4 + 16);
    DeviceColumnView el;
    int64_t kept = n;
    if (n > 0 && !set && !has_nulls) {
      // every row is kept: the sorted column is the element column as it stands
      if (comet_launch_pct_offsets((const uint32_t*)first->p, nullptr, groups, (int32_t*)offs->p, stream_) != 0) throw CometError("collect: launch failed");
      el = val;
      el.valid = nullptr;
      for (auto& o : sorted.owners) out.owners.push_back(o);
    } else {
      DevBuf keep, tiles, C;
      auto idx = std::make_shared<DevBuf>();
      if (n > 0) {
        keep.ensure((size_t)n * 4 + 16);
        tiles.ensure((size_t)((n + 1023) / 1024 + 2) * 8);
        C.ensure((size_t)(n + 2) * 4);
        if (comet_launch_collect_keep(has_nulls ? val.valid : nullptr, set ? (const uint32_t*)fpeer.p : nullptr, n, (uint32_t*)keep.p, stream_) != 0) throw CometError("collect: launch failed");
        pq_launch_u32_scan((const uint32_t*)keep.p, n, (uint64_t*)tiles.p, (int32_t*)C.p, stream_);
        int32_t k32 = 0;
        read_small(&k32, (const char*)C.p + (size_t)n * 4, 4);
        if (k32 < 0 || (int64_t)k32 > n) throw CometError("internal: collect: " + std::to_string(k32) + " kept values over " + std::to_string(n) + " rows");
        kept = k32;
        idx->ensure((size_t)std::max<int64_t>(kept, 1) * 4 + 16);
        if (comet_launch_collect_index((const uint32_t*)keep.p, (const int32_t*)C.p, n, (uint32_t*)idx->p, stream_) != 0) throw CometError("collect: launch failed");
      } else {
        idx->ensure(16);
      }
      if (comet_launch_pct_offsets((const uint32_t*)first->p, n > 0 ? (const int32_t*)C.p : nullptr, groups, (int32_t*)offs->p, stream_) != 0) throw CometError("collect: launch failed");
      bool hv_unused = false;
      el = take_column(val, pl.elem_types[v], false, (const uint32_t*)idx->p, nullptr, kept, hv_unused, out.owners);
      HIP_CHECK(hipStreamSynchronize(stream_));      // flags, counts and row numbers go back to their pools; the sorted column has been read
    }
    DeviceColumnView lv;
    lv.data = offs->p;
    lv.kids.push_back(el);
    lv.kid_has_valid.push_back(0);
    lv.kid_rows = kept;
    for (size_t j = 0; j < nagg; j++)
      if (value_of[j] == (int)v) agg_cols[j] = lv;      // (each aggregate its own state column; equal ones share the buffers)
    out.owners.push_back(offs);
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
    out.types.push_back(list_of(spec.values[(size_t)spec.value_of[j]].elem));
    out.cols.push_back(agg_cols[j]);
    out.has_valid.push_back(false);
  }
  check_device_errors();
  return out;
}

}  // namespace comet
