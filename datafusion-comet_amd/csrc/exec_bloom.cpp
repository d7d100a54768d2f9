// Spark's runtime Bloom filters (InjectRuntimeFilter): bloom_filter_agg as an operator over its materialised child (bloom_kernels.hip), the
// filters that might_contain probes (parsed and checked on the host, uploaded once per context in device/bloom.hpp's layout), and the host
// diagnostics of include/comet_amd.h over the same bloom.hpp code.
// Reference: native/spark-expr/src/bloom_filter/{spark_bloom_filter,spark_bit_array,bloom_filter_agg,bloom_filter_might_contain}.rs.
#include "exec_internal.hpp"
#include "device/bloom.hpp"      // (compiled for the host: comet::bloom_put / bloom_might_contain as the kernels run them)

#include "../../include/comet_amd.h"

extern "C" int comet_launch_bloom_put(const void* vals, int width, const uint8_t* valid_bits, int64_t first, int64_t n, uint64_t* f, int64_t nwords, void* stream);
extern "C" int comet_launch_bloom_merge(const uint8_t* src_words, int64_t nwords, uint64_t* f, void* stream);
extern "C" int comet_launch_bloom_finish(const uint64_t* f, int64_t nwords, uint8_t* out, uint64_t* popcnt, void* stream);

namespace comet {

namespace {

uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

struct BloomHeader {
  int32_t version = 0, k = 0, seed = 0, num_words = 0;
  size_t header_bytes = 0;
};

// the header of a serialized filter, as far as the bytes reach: V1 i32 1 | k | numWords, V2 i32 2 | k | seed | numWords (all big-endian).
// → false: shorter than its header (or than the version word)
bool read_header(const uint8_t* p, size_t len, BloomHeader& h) {
  if (len < 4) return false;
  h.version = (int32_t)be32(p);
  h.header_bytes = h.version == 2 ? 16 : 12;
  if (h.version != 1 && h.version != 2) return true;      // (the caller names the version)
  if (len < h.header_bytes) return false;
  h.k = (int32_t)be32(p + 4);
  h.seed = h.version == 2 ? (int32_t)be32(p + 8) : 0;
  h.num_words = (int32_t)be32(p + h.header_bytes - 4);
  return true;
}

// empty: well-formed; else what is wrong with it
std::string bloom_bytes_problem(const uint8_t* p, size_t len, BloomHeader& h) {
  if (len == 0) return "the filter is empty (0 bytes)";
  if (!read_header(p, len, h)) return "the filter is truncated: " + std::to_string(len) + " bytes do not hold its header";
  if (h.version != 1 && h.version != 2) return "unsupported BloomFilter version " + std::to_string(h.version) + " (expecting 1 or 2)";
  if (h.k < 1 || h.k > kBloomMaxK) return "numHashFunctions " + std::to_string(h.k) + " is outside 1 … " + std::to_string(kBloomMaxK);
  if (h.num_words < 1) return "numWords " + std::to_string(h.num_words) + " is not positive";
  if ((int64_t)h.num_words * 64 >= ((int64_t)1 << 31)) return "numWords " + std::to_string(h.num_words) + " is too large: the bit size must stay below 2^31";
  if (len - h.header_bytes < (size_t)h.num_words * 8)
    return "the filter is truncated: " + std::to_string(len - h.header_bytes) + " bytes of bit array, its header says " + std::to_string((size_t)h.num_words * 8);
  return std::string();
}

// serialized → device/bloom.hpp's layout (header words, then the words in native byte order)
std::vector<uint64_t> to_device_layout(const uint8_t* p, const BloomHeader& h) {
  std::vector<uint64_t> f((size_t)kBloomHeaderWords + (size_t)h.num_words);
  f[0] = (uint64_t)h.version;
  f[1] = (uint64_t)h.k;
  f[2] = (uint64_t)(uint32_t)h.seed;
  f[3] = (uint64_t)h.num_words;
  const uint8_t* w = p + h.header_bytes;
  for (int32_t i = 0; i < h.num_words; i++, w += 8) {
    uint64_t v = 0;
    for (int b = 0; b < 8; b++) v = (v << 8) | w[b];
    f[(size_t)kBloomHeaderWords + (size_t)i] = v;
  }
  return f;
}

// device layout → Spark's serialization
std::string serialize(const std::vector<uint64_t>& f) {
  std::string out;
  auto put32 = [&](uint32_t v) { for (int s = 24; s >= 0; s -= 8) out.push_back((char)(v >> s)); };
  put32((uint32_t)f[0]);
  put32((uint32_t)f[1]);
  if (f[0] == 2) put32((uint32_t)f[2]);
  put32((uint32_t)f[3]);
  for (size_t i = 0; i < (size_t)f[3]; i++) { put32((uint32_t)(f[kBloomHeaderWords + i] >> 32)); put32((uint32_t)f[kBloomHeaderWords + i]); }
  return out;
}

}  // namespace

void bloom_check_bytes(const uint8_t* p, size_t len) {
  BloomHeader h;
  const std::string why = bloom_bytes_problem(p, len, h);
  if (!why.empty()) throw CometError("might_contain: " + why);
}

// bloom_filter_agg's parameters (bloom_filter_agg.rs:56-104): numItems / numBits are Int64 literals truncated to i32, k = max(1, round(numBits / numItems · ln 2))
// with f64::round (half away from zero), numWords = ceil(numBits / 64), seed 0.  Everything this engine refuses is refused here, by name.
BloomAggSpec bloom_agg_spec(const Operator& op) {
  const char* who = "bloom_filter_agg";
  for (auto& x : op.agg_exprs)
    if (x.kind == AggKind::BloomFilter) who = agg_name(x);
  if (!op.grouping_exprs.empty()) throw CometError(std::string(who) + " in a grouped aggregate is not supported by the MI355X native engine (Spark plans it without grouping keys)");
  if (op.agg_exprs.size() != 1) throw CometError(std::string(who) + " mixed with other aggregate functions in one HashAggregate is not supported by the MI355X native engine");
  const AggExpr& a = op.agg_exprs[0];
  if (a.filter) throw CometError(std::string(who) + " with a FILTER (WHERE …) clause is not supported by the MI355X native engine");
  for (int m : op.expr_modes)
    if (m != (int)op.agg_mode) throw CometError(std::string(who) + " in a mixed-mode aggregate is not supported by the MI355X native engine");
  if (a.children.size() != 1) throw CometError(std::string(who) + " expects one child");
  auto i64_lit = [&](const ExprP& e, const char* what) -> int32_t {
    if (!e || e->kind != ExprKind::Literal || e->lit_null || !e->has_dtype || e->dtype.id != TypeId::Int64)
      throw CometError(std::string(who) + ": " + what + " must be an Int64 literal");
    return (int32_t)e->lit_i64;
  };
  const int32_t items = i64_lit(a.bloom_num_items, "numItems"), bits = i64_lit(a.bloom_num_bits, "numBits");
  if (items <= 0) throw CometError(std::string(who) + ": numItems must be positive, got " + std::to_string(items));
  if (bits <= 0) throw CometError(std::string(who) + ": numBits must be positive, got " + std::to_string(bits));
  BloomAggSpec s;
  s.version = a.bloom_version == 2 ? 2 : 1;
  s.num_words = ((int64_t)bits + 63) / 64;
  if (s.num_words * 64 >= ((int64_t)1 << 31)) throw CometError(std::string(who) + ": numBits " + std::to_string(bits) + " rounds up to 2^31 bits or more, which is not supported");
  const double kf = std::round((double)bits / (double)items * std::log(2.0));
  s.k = kf < 1 ? 1 : kf > 2147483647.0 ? 2147483647 : (int)kf;
  if (s.k > kBloomMaxK)
    throw CometError(std::string(who) + ": numBits / numItems gives " + std::to_string(s.k) + " hash functions, more than the " + std::to_string(kBloomMaxK) + " this engine supports");
  return s;
}

bool is_bloom_agg(const Operator& op) {
  if (op.kind != OpKind::HashAgg) return false;
  for (auto& a : op.agg_exprs)
    if (a.kind == AggKind::BloomFilter) return true;
  return false;
}

// ---- the filters might_contain probes ----

const void* ExecutionContext::bloom_buffer(const PipelineDesc::BloomRef& ref) {
  if (!blooms_) blooms_ = std::make_shared<BloomRegistry>();
  const Expr* node = ref.node.get();
  if (ref.subquery_id >= 0) {
    auto it = blooms_->subquery_nodes.find(ref.subquery_id);
    if (it == blooms_->subquery_nodes.end()) throw CometError("might_contain: subquery " + std::to_string(ref.subquery_id) + " has no value yet");
    node = it->second.get();
  }
  auto hit = blooms_->buffers.find(node);
  if (hit != blooms_->buffers.end()) return hit->second->p;
  if (node->kind != ExprKind::Literal || node->lit_null) throw CometError("internal: might_contain bound to a filter without bytes");
  BloomHeader h;
  const uint8_t* p = (const uint8_t*)node->lit_bytes.data();
  const std::string why = bloom_bytes_problem(p, node->lit_bytes.size(), h);
  if (!why.empty()) throw CometError("might_contain: " + why);
  const std::vector<uint64_t> f = to_device_layout(p, h);      // (byte-swapped once, here)
  auto buf = std::make_shared<DevBuf>();
  buf->ensure(f.size() * 8);
  HIP_CHECK(hipMemcpy(buf->p, f.data(), f.size() * 8, hipMemcpyHostToDevice));
  blooms_->buffers[node] = buf;
  blooms_->keep.push_back(ref.node);
  return buf->p;
}

void ExecutionContext::bind_blooms(const PipelineDesc& d, CometKParams& prm) {
  for (size_t j = 0; j < d.blooms.size(); j++) prm.in[COMET_MAX_IN - 1 - j].data = bloom_buffer(d.blooms[j]);
}

// ---- bloom_filter_agg ----

// HashAggregate(keys = [], [bloom_filter_agg(child, numItems, numBits)]) in mode Partial / PartialMerge / Final over its materialised child → one row,
// one Binary column.  Partial: the child expression is evaluated by a fused Projection into one integer column, bloom_put_kernel sets its bits; the state is
// the serialization, never NULL.  PartialMerge / Final: every incoming state row's header is checked on the host against this aggregate's parameters (the
// reference's messages), its words are ORed in; Final yields NULL when no bit is set.
DevTable ExecutionContext::bloom_aggregate(const Operator& op, const DevTable& in) {
  const BloomAggSpec spec = bloom_agg_spec(op);
  const size_t fbytes = ((size_t)kBloomHeaderWords + (size_t)spec.num_words + 1) * 8;      // … + the population count behind the words
  DevBuf acc;
  acc.ensure(fbytes);
  HIP_CHECK(hipMemsetAsync(acc.p, 0, fbytes, stream_));
  const uint64_t header[kBloomHeaderWords] = {(uint64_t)spec.version, (uint64_t)spec.k, 0, (uint64_t)spec.num_words};
  write_small(acc.p, header, sizeof header);
  uint64_t* const f = (uint64_t*)acc.p;
  uint64_t* const popcnt = f + kBloomHeaderWords + spec.num_words;
  if (op.agg_mode == AggMode::Partial) {
    DevTable col = run_chain_to_device(*bloom_proj_.at(&op), in);
    const DType& t = col.types.at(0);
    if (!t.is_integer()) throw CometError("bloom_filter_agg over " + t.str() + " is not supported by the MI355X native engine");
    timed_begin();
    if (comet_launch_bloom_put(col.cols[0].data, fixed_width(t), col.has_valid[0] ? col.cols[0].valid : nullptr, col.cols[0].offset, col.rows, f, spec.num_words, stream_) != 0)
      throw CometError("bloom_filter_agg: launch failed");
    HIP_CHECK(hipStreamSynchronize(stream_));      // col goes out of scope
  } else {
    const size_t sc = (size_t)std::max(0, op.initial_input_buffer_offset);
    if (sc >= in.cols.size() || (in.types[sc].id != TypeId::Bytes && in.types[sc].id != TypeId::String))
      throw CometError("bloom_filter_agg: the merging aggregate expects its Binary state in column " + std::to_string(sc) + " of its child");
    const DeviceColumnView& s = in.cols[sc];
    std::vector<int32_t> offs((size_t)in.rows + 1, 0);
    std::vector<uint8_t> vbits;
    if (in.rows) {
      HIP_CHECK(hipMemcpyAsync(offs.data(), (const int32_t*)s.data + s.offset, offs.size() * 4, hipMemcpyDeviceToHost, stream_));
      if (in.has_valid[sc] && s.valid) {
        vbits.resize((size_t)((s.offset + in.rows + 7) / 8));
        HIP_CHECK(hipMemcpyAsync(vbits.data(), s.valid, vbits.size(), hipMemcpyDeviceToHost, stream_));
      }
      HIP_CHECK(hipStreamSynchronize(stream_));
    }
    timed_begin();
    for (int64_t r = 0; r < in.rows; r++) {
      if (!vbits.empty() && !((vbits[(size_t)((s.offset + r) >> 3)] >> ((s.offset + r) & 7)) & 1)) continue;      // (a NULL state holds nothing)
      const int64_t lo = offs[(size_t)r], len = (int64_t)offs[(size_t)r + 1] - lo;
      if (lo < 0 || len < 0) throw CometError("bloom_filter_agg: the state column's offsets are not ascending");
      // merge_filter (spark_bloom_filter.rs:286-341): the header against this aggregate's own filter, then the length; a few bytes come back per state
      uint8_t hb[16] = {0};
      const size_t have = (size_t)std::min<int64_t>(len, 16);
      if (have) read_small(hb, (const uint8_t*)s.aux + lo, have);
      BloomHeader h;
      if (have < 4) throw CometError("BloomFilter merge: truncated bit array (got 0 bytes, expected " + std::to_string(spec.num_words * 8) + ")");
      h.version = (int32_t)be32(hb);
      if (h.version != spec.version) throw CometError("BloomFilter merge: version mismatch (got " + std::to_string(h.version) + ", expected " + std::to_string(spec.version) + ")");
      if (!read_header(hb, have, h)) throw CometError("BloomFilter merge: truncated bit array (got 0 bytes, expected " + std::to_string(spec.num_words * 8) + ")");
      if (h.k != spec.k) throw CometError("BloomFilter merge: num_hash_functions mismatch (got " + std::to_string((uint32_t)h.k) + ", expected " + std::to_string(spec.k) + ")");
      if (h.seed != 0) throw CometError("BloomFilter merge: seed mismatch (got " + std::to_string(h.seed) + ", expected 0)");
      if ((int64_t)h.num_words != spec.num_words)
        throw CometError("BloomFilter merge: num_words mismatch (got " + std::to_string((uint32_t)h.num_words) + ", expected " + std::to_string(spec.num_words) + ")");
      if (len - (int64_t)h.header_bytes < spec.num_words * 8)
        throw CometError("BloomFilter merge: truncated bit array (got " + std::to_string(len - (int64_t)h.header_bytes) + " bytes, expected " + std::to_string(spec.num_words * 8) + ")");
      if (comet_launch_bloom_merge((const uint8_t*)s.aux + lo + h.header_bytes, spec.num_words, f, stream_) != 0) throw CometError("bloom_filter_agg: launch failed");
    }
  }
  // the serialization, written on the device; the population count decides NULL for Final
  const size_t hdr = spec.version == 2 ? 16 : 12, out_len = hdr + (size_t)spec.num_words * 8;
  auto bytes = std::make_shared<DevBuf>(), out_offs = std::make_shared<DevBuf>();
  bytes->ensure(out_len + 16);
  out_offs->ensure(16);
  if (comet_launch_bloom_finish(f, spec.num_words, (uint8_t*)bytes->p, popcnt, stream_) != 0) throw CometError("bloom_filter_agg: launch failed");
  timed_end();
  uint64_t set_bits = 0;
  read_small(&set_bits, popcnt, 8);
  check_device_errors();
  const bool is_null = op.agg_mode == AggMode::Final && set_bits == 0;
  const int32_t o[2] = {0, is_null ? 0 : (int32_t)out_len};
  write_small(out_offs->p, o, sizeof o);
  DevTable out;
  out.rows = 1;
  out.types.push_back(DType::of(TypeId::Bytes));
  DeviceColumnView v;
  v.data = out_offs->p;
  v.aux = bytes->p;
  out.owners.push_back(out_offs);
  out.owners.push_back(bytes);
  if (is_null) {
    auto vb = std::make_shared<DevBuf>();
    vb->ensure(16);
    const uint8_t zero[8] = {0};
    write_small(vb->p, zero, sizeof zero);
    v.valid = (const uint8_t*)vb->p;
    out.owners.push_back(vb);
  }
  out.cols.push_back(v);
  out.has_valid.push_back(is_null);
  HIP_CHECK(hipStreamSynchronize(stream_));
  return out;
}

}  // namespace comet

// ---- host diagnostics (include/comet_amd.h, COMET_TEST_ABI): the code of device/bloom.hpp, run on the host ----

extern "C" int32_t comet_spark_bloom_might_contain(const uint8_t* bytes, size_t len, int64_t value) {
  comet::BloomHeader h;
  if (!bytes || !comet::bloom_bytes_problem(bytes, len, h).empty()) return -1;
  const std::vector<uint64_t> f = comet::to_device_layout(bytes, h);
  return comet::bloom_might_contain((const comet::u64*)f.data(), (comet::i64)value) ? 1 : 0;
}

extern "C" int64_t comet_spark_bloom_build(const int64_t* values, const uint8_t* valid, int64_t n, int64_t num_items, int64_t num_bits, int32_t version, uint8_t* out, int64_t cap) {
  // the aggregate's own parameter rule, through a one-aggregate HashAggregate node
  comet::Operator op;
  op.kind = comet::OpKind::HashAgg;
  comet::AggExpr a;
  a.kind = comet::AggKind::BloomFilter;
  auto lit = [](int64_t v) {
    auto e = std::make_shared<comet::Expr>();
    e->kind = comet::ExprKind::Literal;
    e->dtype = comet::DType::of(comet::TypeId::Int64);
    e->has_dtype = true;
    e->lit_i64 = v;
    return e;
  };
  a.children.push_back(lit(0));
  a.bloom_num_items = lit(num_items);
  a.bloom_num_bits = lit(num_bits);
  a.bloom_version = version == 2 ? 2 : 1;
  op.agg_exprs.push_back(a);
  comet::BloomAggSpec s;
  try {
    s = comet::bloom_agg_spec(op);
  } catch (const comet::CometError&) {
    return -1;
  }
  std::vector<uint64_t> f((size_t)comet::kBloomHeaderWords + (size_t)s.num_words, 0);
  f[0] = (uint64_t)s.version;
  f[1] = (uint64_t)s.k;
  f[3] = (uint64_t)s.num_words;
  for (int64_t i = 0; i < n; i++)
    if (!valid || ((valid[i >> 3] >> (i & 7)) & 1)) comet::bloom_put((comet::u64*)f.data(), (comet::i64)values[i]);
  const std::string bytes = comet::serialize(f);
  if (out && cap >= (int64_t)bytes.size()) memcpy(out, bytes.data(), bytes.size());
  return (int64_t)bytes.size();
}
