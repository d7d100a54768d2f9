// Hash joins of materialised tables (build, single-pass probe, outer-build tail).
#include "exec_internal.hpp"

namespace comet {
// Join keys that are Utf8 columns with values longer than the 15 bytes of a packed key: an exact string dictionary is built over the
// right column (strdict_kernels.hip), the left column is looked up in it, and the join runs on the two Int64 row-index columns
// instead (a left string without a partner gets a NULL index: NULL keys never match, outer joins still emit the row).  The index
// columns are appended to the inputs and dropped from the result.
DevTable ExecutionContext::hash_join(const Operator& j, const DevTable& L, const DevTable& R) {
  auto is_str = [](const DType& t) { return t.id == TypeId::String || t.id == TypeId::Bytes; };
  std::vector<size_t> sk;
  for (size_t k = 0; k < j.left_keys.size() && k < j.right_keys.size(); k++) {
    const ExprP &a = j.left_keys[k], &b = j.right_keys[k];
    if (a->kind == ExprKind::Bound && b->kind == ExprKind::Bound && a->bound_index >= 0 && b->bound_index >= 0 && (size_t)a->bound_index < L.types.size() &&
        (size_t)b->bound_index < R.types.size() && is_str(L.types[(size_t)a->bound_index]) && is_str(R.types[(size_t)b->bound_index]) &&
        L.cols[(size_t)a->bound_index].offset == 0 && R.cols[(size_t)b->bound_index].offset == 0)
      sk.push_back(k);
  }
  if (sk.empty() || L.rows == 0 || R.rows == 0 || L.cols.size() + R.cols.size() + 2 * sk.size() > COMET_MAX_IN) return hash_join_impl(j, j, L, R, "");
  auto longest = [&](const DevTable& t, int c) {
    uint32_t* mx = (uint32_t*)err_flags_.p + (kErrBytes / 4 - 1);
    HIP_CHECK(hipMemsetAsync(mx, 0, 4, stream_));
    if (comet_launch_str_max_len((const int32_t*)t.cols[(size_t)c].data, t.rows, mx, stream_) != 0) throw CometError("string keys: launch failed");
    uint32_t v = 0;
    read_small(&v, mx, 4);
    HIP_CHECK(hipMemsetAsync(mx, 0, 4, stream_));
    return v;
  };
  bool need = false;
  for (size_t k : sk) need = need || longest(L, j.left_keys[k]->bound_index) > 15 || longest(R, j.right_keys[k]->bound_index) > 15;
  if (!need) return hash_join_impl(j, j, L, R, "");
  if (R.rows >= ((int64_t)1 << 32) - 1) throw CometError("Utf8 join keys longer than 15 bytes over more than 2^32 rows are not supported");
  DevTable l2 = L, r2 = R;
  Operator jj = j;
  for (size_t k : sk) {
    const int lc = j.left_keys[k]->bound_index, rc = j.right_keys[k]->bound_index;
    const DeviceColumnView &lv = L.cols[(size_t)lc], &rv = R.cols[(size_t)rc];
    int64_t slots = 1024;
    while (slots < 2 * R.rows) slots <<= 1;
    DevBuf table;
    table.ensure((size_t)slots * 4);
    HIP_CHECK(hipMemsetAsync(table.p, 0, (size_t)slots * 4, stream_));
    auto rrep = std::make_shared<DevBuf>(), lrep = std::make_shared<DevBuf>(), lbits = std::make_shared<DevBuf>();
    DevBuf lok;
    rrep->ensure((size_t)R.rows * 8 + 16);
    lrep->ensure((size_t)L.rows * 8 + 16);
    lok.ensure((size_t)L.rows + 16);
    lbits->ensure((size_t)((L.rows + 7) / 8) + 16);
    if (comet_launch_str_dict_build((const int32_t*)rv.data, (const uint8_t*)rv.aux, R.has_valid[(size_t)rc] ? rv.valid : nullptr, R.rows, (uint32_t*)table.p, slots,
                                    (int64_t*)rrep->p, stream_) != 0 ||
        comet_launch_str_dict_lookup((const int32_t*)rv.data, (const uint8_t*)rv.aux, (const uint32_t*)table.p, slots, (const int32_t*)lv.data, (const uint8_t*)lv.aux,
                                     L.has_valid[(size_t)lc] ? lv.valid : nullptr, L.rows, (int64_t*)lrep->p, (uint8_t*)lok.p, stream_) != 0)
      throw CometError("string keys: launch failed");
    pq_launch_pack((const uint8_t*)lok.p, (uint8_t*)lbits->p, L.rows, stream_);
    HIP_CHECK(hipStreamSynchronize(stream_));   // `table` and `lok` go back to the pool
    DeviceColumnView rid, lid;
    rid.data = rrep->p;
    rid.valid = rv.valid;
    lid.data = lrep->p;
    lid.valid = (const uint8_t*)lbits->p;
    jj.right_keys[k] = bound((int)r2.cols.size(), DType::of(TypeId::Int64));
    jj.left_keys[k] = bound((int)l2.cols.size(), DType::of(TypeId::Int64));
    r2.types.push_back(DType::of(TypeId::Int64));
    r2.cols.push_back(rid);
    r2.has_valid.push_back(R.has_valid[(size_t)rc]);
    r2.owners.push_back(rrep);
    l2.types.push_back(DType::of(TypeId::Int64));
    l2.cols.push_back(lid);
    l2.has_valid.push_back(true);
    l2.owners.push_back(lrep);
    l2.owners.push_back(lbits);
  }
  const size_t nl = L.cols.size(), nr = R.cols.size(), extra = sk.size();
  // the residual condition addresses left ++ right: the right columns moved up by the index columns appended to the left
  if (jj.join_condition) jj.join_condition = shift_bound(j.join_condition, (int)extra, (int)nl);
  DevTable out = hash_join_impl(j, jj, l2, r2, ":SD");
  // drop the index columns: the result is left' ++ right' (semi / anti joins: left' only)
  auto drop = [&](size_t first, size_t count) {
    if (first + count > out.cols.size()) return;
    out.types.erase(out.types.begin() + (long)first, out.types.begin() + (long)(first + count));
    out.cols.erase(out.cols.begin() + (long)first, out.cols.begin() + (long)(first + count));
    out.has_valid.erase(out.has_valid.begin() + (long)first, out.has_valid.begin() + (long)(first + count));
  };
  if (out.cols.size() == nl + extra + nr + extra) drop(nl + extra + nr, extra);
  else if (out.cols.size() != nl + extra) throw CometError("internal: unexpected join output width with string keys");
  drop(nl, extra);
  return out;
}

namespace {
// ---- the join kernels' arguments, named on the host side.  The device side reads the same slots in comet_device.hpp (the name or the body that
// does is given with each); one definition for both sides, in kparams.h, is a follow-up. ----
// prm.out[] beside kOutErr and the output columns from kOutFirstCol on:
constexpr int kJoinOutTable = 0;        // out[0]: chained heads (join_build_body `head`) / bucket table (join_table_build_body `tab`) / direct-map ranks (JoinDirectTable) / k_jbcnt's counters (`total`)
constexpr int kJoinOutRows = 1;         // out[1]: chained next[] (`next`) / the bucket table's partition records (`recs`) / the direct map's rows[] in key order (`rows`)
constexpr int kJoinOutParts = 3;        // out[3]: partition starts, totals, monotone-hash words, per-block counts (`pstart`, kJoinPartTotOff, kJoinPartMono, kJoinPartCntOff)
constexpr int kJoinOutKeyMap = 44;      // kJoinKeyMap
constexpr int kJoinOutMatched = 45;     // kJoinMatched
constexpr int kJoinOutBuildTiles = 46;  // kJoinBuildTiles
constexpr int kJoinOutCounters = 47;    // the counter block: join_probe_tiles `emitted`, join_sample_table `cnt`, the flags below
// u64 words of the counter block (64 bytes)
constexpr int kCntEmitted = 0;          // probe: emitted rows; k_jbcnt: run leaders; sample: probe rows asked
constexpr int kCntKeyMin = 1;           // k_jbcnt: smallest key, order-preserving u64 (sign bit flipped); sample: rows with a partner
constexpr int kCntKeyMax = 2;           // k_jbcnt: largest key
constexpr int kCntKeyedRows = 3;        // k_jbcnt: rows with a non-NULL key
constexpr int kCntKeyTwice = 4;         // k_jbmap / k_jdrows: "a key came twice" (join_keymap_build_body `flag`)
constexpr int kCntOverflow = 6;         // k_jtbuild, the partition scan: "a bucket-table partition overflowed"
// prm.iarg[]: slots 0, 2, 5 and 6 mean different things to different kernels, so each family has its setter and a launch site says what it passes
constexpr int kJoinArgBuildRows = 1;    // `nb` of every build body
constexpr int kJoinArgBuildTiles = 3;   // k_jbscan: tiles of 1 024 build rows
constexpr int kJoinArgTailBase = 4;     // k_jbemit: the output row of the first unmatched build row
inline void chained_table_args(CometKParams& prm, int64_t capacity, int index_bits) { prm.iarg[0] = capacity; prm.iarg[2] = index_bits; }      // JoinGlobalTable: mask + 1, `ib`
inline void bucket_table_args(CometKParams& prm, int64_t slots, int64_t partitions, int64_t scatter_chunk) {      // join_part_hist_body `slots`, `np`, `chunk`
  prm.iarg[0] = slots;
  prm.iarg[2] = partitions;
  prm.iarg[5] = scatter_chunk;
}
inline void keymap_build_args(CometKParams& prm, bool want_dup_flag) { prm.iarg[5] = want_dup_flag ? 1 : 0; }      // join_keymap_build_body (0: the wave-combined build, which cannot tell)
inline void direct_rows_args(CometKParams& prm, int64_t keyed_rows) { prm.iarg[6] = keyed_rows; }                 // join_direct_rows_body compares the bitmap's bit count with it: fewer bits = a key came twice
inline void sample_args(CometKParams& prm, int64_t sample_rows) { prm.iarg[5] = sample_rows; }                    // join_sample_table `ns`
inline void probe_args(CometKParams& prm, int64_t out_capacity) { prm.iarg[6] = out_capacity; }                   // join_probe_tiles `cap_out`

// The switches of the join's host side, read once per process (INTEGRATION.md lists them)
struct JoinSettings {
  int64_t bucket_min_rows = 65536;      // COMET_JOIN_BUCKET_MIN_ROWS: build sides from this many rows on get the bucket table (negative: never)
  int mono = 1;                         // COMET_JOIN_MONO: 0 = never the monotone hash
  int bitmap_only = 1;                  // COMET_JOIN_BITMAP_ONLY: 0 = semi / anti joins build a table even where the bitmap would answer
  int direct = 1;                       // COMET_JOIN_DIRECT: 0 = never the direct map
  int keymap = -1;                      // COMET_JOIN_KEYMAP: 0 never, 1 always, default: by the sample
  bool debug = false;                   // COMET_JOIN_DEBUG: what the build count found, on stderr
  static const JoinSettings& get() {
    static const JoinSettings s = [] {
      JoinSettings r;
      if (const char* e = getenv("COMET_JOIN_BUCKET_MIN_ROWS")) r.bucket_min_rows = atoll(e);
      if (const char* e = getenv("COMET_JOIN_MONO")) r.mono = atoi(e);
      if (const char* e = getenv("COMET_JOIN_BITMAP_ONLY")) r.bitmap_only = atoi(e);
      if (const char* e = getenv("COMET_JOIN_DIRECT")) r.direct = atoi(e);
      if (const char* e = getenv("COMET_JOIN_KEYMAP")) r.keymap = atoi(e);
      r.debug = getenv("COMET_JOIN_DEBUG") != nullptr;
      return r;
    }();
    return s;
  }
};

enum class JoinTable { Lds, Chained, Bucket, Direct, BitmapOnly };

// (k_jprobe_km / k_jprobe_bkm: the table probes that ask the key bitmap first; without a bitmap the leaner ones — comet_device.hpp join_probe_tiles)
inline const char* probe_kernel(JoinTable t, bool keymap_built) {
  switch (t) {
    case JoinTable::Lds: return "k_jlds";
    case JoinTable::BitmapOnly: return "k_jprobe_bm";
    case JoinTable::Direct: return "k_jdprobe";
    case JoinTable::Bucket: return keymap_built ? "k_jprobe_bkm" : "k_jprobe_b";
    default: return keymap_built ? "k_jprobe_km" : "k_jprobe";
  }
}

// what counting the build side found (count_build; without it: one entry per row, nothing known about the keys)
struct BuildStats {
  int64_t entries = 0, keyed_rows = -1;               // runs of equal neighbouring keys; rows with a non-NULL key
  uint64_t key_first = 0, key_range = 0;              // one integer key's range whatever its density (the monotone hash of the bucket table; 0: none / unknown)
  uint64_t keymap_first = 0, keymap_range = 0;        // … where it is a candidate for the key bitmap: values spanning a foreign key's range
};

}  // namespace

// One attempt at one join: plan, count, build one of the tables, probe, the build side's tail, the result table.  ONE CometKParams is filled in place across the
// launches: later kernels see what earlier steps set (iarg[5] left at the scatter chunk, out[0] / out[1] re-pointed from the direct map to the bucket table
// when a key turned out to come twice).  Every buffer is a member: nothing returns to the pool before the run ends, whatever is still queued on the stream.
struct HashJoinRun {
  ExecutionContext& cx;
  const Operator &node, &j;
  const DevTable &L, &R, &B, &P;      // B / P: the build and the probe side among L / R
  const std::string& key_suffix;
  const JoinFusion *fused_probe, *fused_build;
  const bool allow_bucket;
  const JoinSettings& set = JoinSettings::get();
  const int64_t n;                    // probe rows
  Variant v;
  CometKParams prm;
  DevBuf head, next, matched, btiles, counters, keymap, dranks, drows, dtiles, dcounts, btab, brecs, bpart;
  std::vector<std::shared_ptr<DevBuf>> vals, vbytes;
  JoinTable table = JoinTable::Chained;
  bool keymap_built = false;
  BuildStats st;
  int64_t nbtiles = 0, out_rows = 0, tail_rows = 0, probe_capacity = 0;

  HashJoinRun(ExecutionContext& cx, const Operator& node, const Operator& j, const DevTable& L, const DevTable& R, const std::string& key_suffix, const JoinFusion* fused_probe,
              const JoinFusion* fused_build, bool allow_bucket)
      : cx(cx), node(node), j(j), L(L), R(R), B(j.build_side == BuildSide::Left ? L : R), P(j.build_side == BuildSide::Left ? R : L), key_suffix(key_suffix), fused_probe(fused_probe),
        fused_build(fused_build), allow_bucket(allow_bucket), n(P.rows) {}

  hipStream_t stream() const { return cx.stream_; }
  int build_grid() const { return (int)std::min<int64_t>((B.rows + 255) / 256, 256 * 8); }
  void* counter(int word) const { return (char*)counters.p + 8 * word; }

  // planned once per (join node, validity patterns); the kernel arguments every launch shares
  void plan() {
    v = cx.node_variant(node, ":J:", validity_key(L.has_valid) + "|" + validity_key(R.has_valid) + key_suffix,
                        [&] { return generate_join(j, L.types, R.types, L.has_valid, R.has_valid, fused_probe, fused_build); });
    if (B.rows >= ((int64_t)1 << 31)) throw CometError("hash join build side exceeds 2^31 rows");
    memset(&prm, 0, sizeof prm);
    bind_inputs(prm, B.cols, B.has_valid);
    bind_inputs(prm, P.cols, P.has_valid, B.cols.size());
    counters.ensure(64);
    HIP_CHECK(hipMemsetAsync(counters.p, 0, 64, stream()));
    prm.n = n;
    prm.iarg[kJoinArgBuildRows] = B.rows;
    st.entries = B.rows;
  }

  // The bucket array holds one entry per RUN of equal neighbouring keys (comet_device.hpp "Runs of equal keys"), not one per row: a large
  // build side is counted first (one coalesced pass over its key columns) so that a clustered fact table — several rows per key — gets
  // a bucket array sized by its runs, which stays in the caches several times better than one sized by its rows.
  void count_build() {
    // leaders, smallest key, largest key (order-preserving u64), rows with a non-NULL key
    HIP_CHECK(hipMemsetAsync(counter(kCntKeyMin), 0xff, 8, stream()));
    prm.out[kJoinOutTable] = counters.p;
    prm.out[kOutErr] = cx.err_flags_.p;
    cx.launch(v, "k_jbcnt", build_grid(), prm);
    uint64_t got[4] = {0, 0, 0, 0};
    cx.read_small(got, counters.p, sizeof got);
    st.entries = std::min<int64_t>(B.rows, (int64_t)got[kCntEmitted]);
    st.keyed_rows = (int64_t)got[kCntKeyedRows];
    const uint64_t lo = got[kCntKeyMin], hi = got[kCntKeyMax];
    if (set.debug)
      fprintf(stderr, "[join %s] build rows %lld: leaders %llu, keyed rows %llu, key min %lld max %lld\n", key_suffix.c_str(), (long long)B.rows, (unsigned long long)got[kCntEmitted],
              (unsigned long long)got[kCntKeyedRows], (long long)(lo ^ ((uint64_t)1 << 63)), (long long)(hi ^ ((uint64_t)1 << 63)));
    // The key bitmap (comet_device.hpp kJoinKeyMap): one integer key whose values span at most 64 bits per build row and 2^31 bits — a
    // foreign key's shape.  k_jbcnt leaves min / max untouched when the kernel has no such key (KEYMAP false).
    if (lo > hi) return;
    const uint64_t range = hi - lo + 1;      // (never 0: the keys are 64-bit values of ≤ 2^31 rows … guarded anyway)
    if (range == 0) return;
    st.key_first = lo ^ ((uint64_t)1 << 63);
    st.key_range = range;
    if (range <= ((uint64_t)1 << 31) && range <= (uint64_t)B.rows * 64) {
      st.keymap_first = st.key_first;
      st.keymap_range = range;
    }
  }

  void build_keymap(bool want_dup_flag) {
    const size_t words = (size_t)((st.keymap_range + 127) / 128) * 4;       // whole 128-bit blocks
    keymap.ensure(16 + words * 4 + 16);
    HIP_CHECK(hipMemsetAsync((char*)keymap.p + 16, 0, words * 4 + 16, stream()));
    const uint64_t hdr[2] = {st.keymap_first, st.keymap_range};
    cx.write_small(keymap.p, hdr, sizeof hdr);
    HIP_CHECK(hipMemsetAsync(counter(kCntKeyTwice), 0, 8, stream()));
    keymap_build_args(prm, want_dup_flag);
    prm.out[kJoinOutKeyMap] = keymap.p;
    prm.out[kJoinOutCounters] = counters.p;
    prm.out[kOutErr] = cx.err_flags_.p;
    cx.launch(v, "k_jbmap", build_grid(), prm);
    cx.join_keymap_bytes_ += (int64_t)words * 4;      // (a join that runs twice — the bucket-overflow fallback — counts both attempts here, in join_direct_maps_ and in the kernel times)
    keymap_built = true;
  }

  // The DIRECT MAP (comet_device.hpp JoinDirectTable): when the bitmap's key is also UNIQUE — every build row leads its own run, and the bitmap's build
  // pass sees no bit twice — the bitmap, the keys below each of its 128-bit blocks and the build rows in key order replace the hash table.
  bool try_direct() {
    build_keymap(false);      // (the wave-combined build: duplicates show as missing bits, counted below)
    // ranks and rows[] are built right behind the bitmap, BEFORE the host knows whether a key came twice (one wait instead of three; with a duplicate the
    // two small passes were for nothing — their writes stay inside their buffers either way)
    const int64_t nblocks = (int64_t)((st.keymap_range + 127) / 128);
    dcounts.ensure((size_t)nblocks * 4 + 16);
    dranks.ensure((size_t)(nblocks + 2) * 4);
    dtiles.ensure((size_t)((nblocks + 1023) / 1024 + 2) * 8);
    drows.ensure((size_t)B.rows * 4 + 16);
    if (comet_launch_popcount128((const char*)keymap.p + 16, nblocks, (uint32_t*)dcounts.p, stream()) != 0) throw CometError("hash join: launch failed");
    pq_launch_u32_scan((const uint32_t*)dcounts.p, nblocks, (uint64_t*)dtiles.p, (int32_t*)dranks.p, stream());
    prm.out[kJoinOutTable] = dranks.p;
    prm.out[kJoinOutRows] = drows.p;
    direct_rows_args(prm, st.keyed_rows);
    cx.launch(v, "k_jdrows", build_grid(), prm);
    uint64_t dup = 1;
    cx.read_small(&dup, counter(kCntKeyTwice), 8);
    if (dup) return false;
    cx.join_direct_maps_++;
    return true;
  }

  // The general table (comet_device.hpp template D''): partition passes, then the LDS build — 16-byte entries, one random access per probe key.
  // false: more runs than 16384 partitions hold (the chained table takes the join)
  bool build_bucket() {
    constexpr int64_t kS = 4096, kMaxP = 16384;            // comet_device.hpp kJoinPartSlots, kJoinPartMax
    const int64_t np = std::max<int64_t>(1, (std::max<int64_t>(st.entries, 1) + kS / 2 - 1) / (kS / 2));
    if (np > kMaxP) return false;
    const int64_t g = std::min<int64_t>(256, (B.rows + 4095) / 4096);
    const int64_t chunk = ((B.rows + g - 1) / g + 1023) / 1024 * 1024;
    const int64_t bslots = np * kS;
    btab.ensure((size_t)bslots * 16);
    brecs.ensure((size_t)std::max<int64_t>(st.entries, 1) * 16 + 16);
    bpart.ensure((size_t)(2 * kMaxP + 16 + g * np) * 4 + 16);
    bucket_table_args(prm, bslots, np, chunk);
    prm.out[kJoinOutTable] = btab.p;
    prm.out[kJoinOutRows] = brecs.p;
    prm.out[kJoinOutParts] = bpart.p;
    prm.out[kJoinOutCounters] = counters.p;
    prm.out[kOutErr] = cx.err_flags_.p;
    // The monotone hash (comet_device.hpp join_mono_hash) where the key is one integer with a known range: slots in key order.  Whether the keys are spread
    // evenly enough is asked BEFORE the table is built (a partition above 7/8 of its slots: the scan kernel's flag, one word read back) — if not, the
    // scrambling hash, whose own overflow (many separate runs of one key) is only read with the probe's result.
    bool mono = set.mono != 0 && st.key_range != 0;
    for (;;) {
      const uint64_t mp[3] = {mono ? (~(uint64_t)0) / st.key_range : 0, st.key_first, st.key_range};      // (⌊(2^64 − 1) / range⌋ ≤ ⌊2^64 / range⌋: still injective, still below all ones)
      cx.write_small((uint32_t*)bpart.p + (kMaxP + 4), mp, sizeof mp);
      cx.launch(v, "k_jphist", (int)g, prm, 1024);
      if (comet_launch_join_part_scan((uint32_t*)bpart.p + (2 * kMaxP + 16), (int)g, (int)np, (uint32_t*)bpart.p + (kMaxP + 16), (uint32_t)(kS - kS / 8), (uint64_t*)counter(kCntOverflow),
                                      stream()) != 0)
        throw CometError("hash join: launch failed");
      if (!mono) break;
      uint64_t over = 0;
      cx.read_small(&over, counter(kCntOverflow), 8);
      if (!over) break;
      mono = false;
      HIP_CHECK(hipMemsetAsync(counter(kCntOverflow), 0, 8, stream()));
    }
    cx.launch(v, "k_jpscat", (int)g, prm, 1024);
    cx.launch(v, "k_jtbuild", (int)np, prm);
    cx.join_bucket_tables_++;
    if (mono) cx.join_mono_tables_++;
    return true;
  }

  // Small build sides keep the chained table (it sits in L2, and one launch builds it); so does a build side with more runs than the bucket table's partitions hold.
  // The LDS probe's arguments are the chained table's (its buffers are allocated, not built).  Also here: what an outer join's build-side tail needs.
  void build_chained() {
    const bool chained = table == JoinTable::Lds || table == JoinTable::Chained;
    int64_t cap = 1024;
    if (chained) {
      while (cap < 2 * st.entries) cap <<= 1;
      head.ensure((size_t)cap * 4);     // u32 per bucket: newest run leader | tag | "more than one row" flag (comet_device.hpp template D)
      next.ensure((size_t)std::max<int64_t>(B.rows, 1) * 4 + 16);
      HIP_CHECK(hipMemsetAsync(head.p, 0xff, (size_t)cap * 4, stream()));
    }
    nbtiles = (B.rows + 1023) / 1024;
    if (v.desc.join_outer_build) {
      matched.ensure((size_t)std::max<int64_t>(B.rows, 1));
      btiles.ensure((size_t)(nbtiles + 1) * 8);
      HIP_CHECK(hipMemsetAsync(matched.p, 0, (size_t)std::max<int64_t>(B.rows, 1), stream()));
      prm.out[kJoinOutMatched] = matched.p;
      prm.out[kJoinOutBuildTiles] = btiles.p;
      prm.iarg[kJoinArgBuildTiles] = nbtiles;
    }
    if (table != JoinTable::Bucket) {      // (the direct map's and the bitmap's kernels read neither)
      int ib = 1;                          // bits of a build row index: rows ≤ 2^ib − 1, so an index is never all ones
      while (ib < 31 && ((int64_t)1 << ib) - 1 < std::max<int64_t>(B.rows, 1)) ib++;
      if (((int64_t)1 << ib) - 1 < B.rows) throw CometError("HashJoin: build sides of 2^31 rows or more are not supported");
      chained_table_args(prm, cap, ib);
    }
    if (chained) {
      prm.out[kJoinOutTable] = head.p;
      prm.out[kJoinOutRows] = next.p;
    }
    prm.out[kOutErr] = cx.err_flags_.p;
    cx.timed_begin();
    if (table == JoinTable::Chained && B.rows) cx.launch(v, "k_jbuild", build_grid(), prm);
    prm.out[kJoinOutCounters] = counters.p;
  }

  // The key bitmap (comet_device.hpp kJoinKeyMap) pays when probe rows miss: 8192 probe rows, evenly spaced, go through the finished table
  // first; fewer than half with a partner → one more pass over the build keys sets the bits, and the probe asks them before the table.
  // (… and only where the probe side is several times the build side: the bitmap's build pass costs what the build side's atomics cost —
  // 2.2 ms for each of TPC-DS Q95's 70 M-row builds, whose equally large probe sides it did not speed up)
  void maybe_sample_keymap() {
    // (the bitmap is the table; the direct map holds it; or it exists already — the build side turned out not to be unique — and filters the probe rows as below)
    if (table == JoinTable::BitmapOnly || table == JoinTable::Direct || keymap_built) return;
    if (!(st.keymap_range && set.keymap != 0 && n >= (1 << 20) && (set.keymap == 1 || n >= 4 * B.rows))) return;
    bool wanted = set.keymap == 1;
    if (!wanted) {
      HIP_CHECK(hipMemsetAsync(counters.p, 0, 16, stream()));
      const int64_t ns = 8192;
      sample_args(prm, ns);
      cx.launch(v, table == JoinTable::Bucket ? "k_jsample_b" : "k_jsample", (int)((ns + 255) / 256), prm);
      uint64_t cnt[2] = {0, 0};
      cx.read_small(cnt, counters.p, sizeof cnt);
      wanted = cnt[0] >= 64 && cnt[1] * 2 < cnt[0];
    }
    if (wanted) build_keymap(false);
  }

  void bind_outputs(int64_t rows_cap) {
    const PipelineDesc& d = v.desc;
    for (size_t c = 0; c < d.out_cols.size(); c++) {
      if (!vals[c]) vals[c] = std::make_shared<DevBuf>();
      vals[c]->ensure((size_t)std::max<int64_t>(rows_cap, 1) * out_width(d.out_cols[c]) + 16);
      prm.out[kOutFirstCol + 2 * c] = vals[c]->p;
      if (!vbytes[c]) vbytes[c] = std::make_shared<DevBuf>();
      if (d.out_cols[c].nullable) {
        vbytes[c]->ensure((size_t)std::max<int64_t>(rows_cap, 1) + 16);
        prm.out[kOutFirstCol + 2 * c + 1] = vbytes[c]->p;
      }
    }
  }

  // ---- single-pass probe (comet_device.hpp template D'): a small build side is hashed into LDS by every block, a large one sits in its global
  // table; either way the probe counts and emits in one launch, reserving output ranges with one atomic per tile ----
  // false: a partition of the bucket table overflowed (many separate runs of one key) — the stream is idle, this run's tables may go
  bool probe() {
    const PipelineDesc& d = v.desc;
    // FK-shaped joins emit at most one row per probe row; anything beyond the capacity is counted, not written, and the probe re-run
    int64_t out_cap = d.join_build_only ? 1 : n + 1024;
    for (int attempt = 0; n > 0; attempt++) {
      bind_outputs(out_cap);
      probe_args(prm, out_cap);
      HIP_CHECK(hipMemsetAsync(counter(kCntEmitted), 0, 8, stream()));
      const int64_t ptiles = (n + 4095) / 4096;      // kJoinR0 × 256 probe rows per tile (comet_device.hpp)
      cx.launch(v, probe_kernel(table, keymap_built), (int)std::min<int64_t>(ptiles, table == JoinTable::Lds ? 256 * 3 : 256 * 8), prm);
      uint64_t words[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      cx.read_small(words, counters.p, sizeof words);
      if (table == JoinTable::Bucket && words[kCntOverflow]) {
        cx.timed_end();
        HIP_CHECK(hipStreamSynchronize(stream()));
        cx.join_bucket_tables_--;
        return false;
      }
      out_rows = d.join_build_only ? 0 : (int64_t)words[kCntEmitted];
      if (out_rows <= out_cap) break;
      if (attempt == 1) throw CometError("internal: hash join output exceeded its exact size");
      out_cap = out_rows;
    }
    probe_capacity = n > 0 ? out_cap : 0;
    return true;
  }

  // build rows without a match follow the probe-driven rows: count, scan, grow the output where it is too small (keeping what the probe wrote), emit
  void outer_tail() {
    const PipelineDesc& d = v.desc;
    const size_t ncol = d.out_cols.size();
    if (d.join_outer_build && B.rows > 0) {
      cx.launch(v, "k_jbcount", (int)std::min<int64_t>(nbtiles, 256 * 8), prm);
      cx.launch(v, "k_jbscan", 1, prm);
      uint64_t total = 0;
      cx.read_small(&total, (char*)btiles.p + (size_t)nbtiles * 8, 8);
      tail_rows = (int64_t)total;
      prm.iarg[kJoinArgTailBase] = out_rows;
    }
    const int64_t all_rows = out_rows + tail_rows;
    if (all_rows > probe_capacity || (ncol > 0 && !vals[0])) {
      std::vector<std::shared_ptr<DevBuf>> ov = vals, ob = vbytes;
      for (size_t c = 0; c < ncol; c++) { vals[c].reset(); vbytes[c].reset(); }
      bind_outputs(all_rows);
      for (size_t c = 0; c < ncol && out_rows > 0; c++) {
        HIP_CHECK(hipMemcpyAsync(vals[c]->p, ov[c]->p, (size_t)out_rows * out_width(d.out_cols[c]), hipMemcpyDeviceToDevice, stream()));
        if (d.out_cols[c].nullable) HIP_CHECK(hipMemcpyAsync(vbytes[c]->p, ob[c]->p, (size_t)out_rows, hipMemcpyDeviceToDevice, stream()));
      }
      HIP_CHECK(hipStreamSynchronize(stream()));   // the old buffers return to the pool
    }
    if (tail_rows > 0) cx.launch(v, "k_jbemit", (int)std::min<int64_t>(nbtiles, 256 * 8), prm);
    cx.timed_end();
    out_rows = all_rows;
  }

  DevTable finish() {
    // gathered Utf8 payload columns name their source by its kernel-argument index: build columns, then probe columns
    const int nbuild = (int)B.cols.size();
    DevTable out = cx.outputs_to_table(v, vals, vbytes, out_rows, [&](int c) { return c < nbuild ? std::make_pair(&B, c) : std::make_pair(&P, c - nbuild); });
    if (fused_probe || fused_build) cx.check_device_errors();     // the chain's expressions may raise ANSI errors; an unfused chain checks after its own launch
    // the tables of this run (heads, records, bitmap, ranks …) go back to the pool when it ends: nothing queued may still read them.  The probe's result was
    // waited for (read_small) and only the output's own buffers are touched after it — except by the build-side tail of an outer join, and when no probe ran.
    // (ADVICE item 2 is about this condition; it is kept as it was)
    if (tail_rows > 0 || n == 0) HIP_CHECK(hipStreamSynchronize(stream()));
    out.owners.push_back(v.mod);
    cx.join_build_rows_ += B.rows;
    cx.join_probe_rows_ += P.rows;
    return out;
  }

  // false: the bucket table overflowed and the join has to run again without it
  bool run() {
    plan();
    const bool use_lds = B.rows > 0 && B.rows <= 6144;
    bool bucket = !use_lds && allow_bucket && set.bucket_min_rows >= 0 && B.rows >= set.bucket_min_rows;
    // (run counting: from 65536 rows on where the bucket table may take the join, from 2^20 on for the chained table — a join that runs again
    // without the bucket table decides by the second threshold)
    if (!use_lds && B.rows >= (bucket ? 65536 : (1 << 20))) count_build();
    table = use_lds ? JoinTable::Lds : JoinTable::Chained;
    // A semi / anti join that only asks whether the key exists (no residual, probe rows kept) over a bitmap's key: the bitmap is the whole build side.
    if (st.keymap_range != 0 && v.desc.join_dedup_build && set.bitmap_only != 0 && n > 0) {
      build_keymap(false);
      table = JoinTable::BitmapOnly;
      cx.join_bitmap_only_++;
    } else if (st.keymap_range && set.direct != 0 && st.entries == st.keyed_rows) {       // (no two neighbouring rows share a key: a clustered fact table is spared the pass)
      if (try_direct()) table = JoinTable::Direct;
    }
    if (bucket && table == JoinTable::Chained && B.rows != 0 && build_bucket()) table = JoinTable::Bucket;
    vals.resize(v.desc.out_cols.size());
    vbytes.resize(v.desc.out_cols.size());
    build_chained();
    maybe_sample_keymap();
    if (!probe()) return false;
    outer_tail();
    return true;
  }
};

DevTable ExecutionContext::hash_join_impl(const Operator& node, const Operator& j, const DevTable& L, const DevTable& R, const std::string& key_suffix,
                                          const JoinFusion* fused_probe, const JoinFusion* fused_build) {
  // with `fused_build` the build-side table (L when the build side is left) is the SOURCE of the build chain
  // with `fused_probe` the probe-side table (R when the build side is left) is the SOURCE of the probe chain
  // First with the bucket table allowed.  That one of its partitions overflowed is only read with the probe's result: the join then runs again over the
  // chained table (the first run waited for the stream, its tables go back to the pool with it).
  for (bool allow_bucket : {true, false}) {
    HashJoinRun run(*this, node, j, L, R, key_suffix, fused_probe, fused_build, allow_bucket);
    if (run.run()) return run.finish();
  }
  throw CometError("internal: a hash join without a bucket table reported a bucket overflow");
}

}  // namespace comet
