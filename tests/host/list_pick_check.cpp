// csrc/device/list_pick.hpp — the per-element code of array_remove / array_compact / slice / reverse of an array / array_join that list_pick_kernels.hip runs
// on the device — over random list columns against a naive per-list check, in the kernels' own steps: one pass over the ELEMENT rows with lf_list_of, the
// flags' and the lengths' scans, the bytes.  Every buffer is a vector of exactly the bytes Arrow would hand over — the joined string's too —, so a read or a write
// past an end is an AddressSanitizer report.  Built with -fsanitize=address,undefined by tests/test_list_pick_cpu.py and run on the CPU; prints "ok" and exits 0
// when every answer was right.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "device/list_pick.hpp"

namespace {

struct Column {      // several lists laid end to end, as a list column's element column is
  int kind = LF_I64;
  bool with_nulls = false;
  std::vector<uint8_t> data, aux, valid;
  std::vector<int32_t> offs;      // the lists' offsets
  std::vector<bool> is_null;
  std::vector<std::string> text;      // LF_STR: the values
  std::vector<__int128> num;          // the others
  LfCol view() const {
    LfCol c;
    c.data = data.data();
    c.aux = aux.empty() ? nullptr : aux.data();
    c.valid = valid.empty() ? nullptr : valid.data();
    c.offset = 0;
    c.kind = kind;
    return c;
  }
  void build() {
    const size_t n = is_null.size();
    if (with_nulls) {
      valid.assign((n + 7) / 8, 0);
      for (size_t i = 0; i < n; i++)
        if (!is_null[i]) valid[i >> 3] |= (uint8_t)(1u << (i & 7));
    }
    if (kind == LF_STR) {
      std::vector<int32_t> so(1, 0);
      for (auto& s : text) {
        aux.insert(aux.end(), s.begin(), s.end());
        so.push_back((int32_t)aux.size());
      }
      data.resize(so.size() * 4);
      memcpy(data.data(), so.data(), data.size());
    } else if (kind == LF_BOOL) {
      data.assign((n + 7) / 8, 0);
      for (size_t i = 0; i < n; i++)
        if (num[i]) data[i >> 3] |= (uint8_t)(1u << (i & 7));
    } else {
      data.resize(n * (size_t)kind);
      for (size_t i = 0; i < n; i++) memcpy(data.data() + i * (size_t)kind, &num[i], (size_t)kind);      // little endian
    }
    if (data.empty()) data.resize(1);
  }
  bool same(size_t i, size_t j) const { return kind == LF_STR ? text[i] == text[j] : num[i] == num[j]; }
};

const char* const kWords[] = {"", "a", "ab", "abcdefgh", "abcdefghi", "abcdefghj", "abcdefgh\x01", "\xe6\x97\xa5", "\xff", "zzzzzzzzzzzzzzzzzzzz", "zzzzzzzzzzzzzzzzzzzy"};

void push_value(std::mt19937_64& rng, Column& c) {
  if (c.kind == LF_STR) {
    std::string s = kWords[rng() % 11];
    if (rng() % 7 == 0) s.push_back('\0');      // a value that is another plus a zero byte: equal zero-padded prefixes
    c.text.push_back(s);
    c.num.push_back(0);
    return;
  }
  __int128 v = (__int128)(int64_t)(rng() % 5) - 2;
  const int pick = (int)(rng() % 9);
  const int bits = c.kind == LF_BOOL ? 1 : c.kind == LF_I128 ? 127 : c.kind * 8;
  if (c.kind == LF_BOOL) v = (int)(rng() & 1);
  else if (pick == 0) v = -((__int128)1 << (bits - 1));
  else if (pick == 1) v = ((__int128)1 << (bits - 1)) - 1;
  else if (pick == 2 && c.kind == LF_I128) v = ((__int128)1 << 64) + (int64_t)(rng() % 3);
  c.num.push_back(v);
  c.text.emplace_back();
}

Column make(std::mt19937_64& rng, int kind, int nlists, int max_len, bool with_nulls) {
  Column c;
  c.kind = kind;
  c.with_nulls = with_nulls;
  c.offs.push_back(0);
  for (int l = 0; l < nlists; l++) {
    const int n = (int)(rng() % (uint64_t)(max_len + 1));
    for (int i = 0; i < n; i++) {
      c.is_null.push_back(with_nulls && rng() % 4 == 0);
      push_value(rng, c);
    }
    c.offs.push_back((int32_t)c.is_null.size());
  }
  c.build();
  return c;
}

int fails = 0;
void expect(bool ok, const char* what, int kind, long long at) {
  if (ok) return;
  if (fails++ < 20) fprintf(stderr, "FAIL %s (kind %d, at %lld)\n", what, kind, at);
}

void check_kind(std::mt19937_64& rng, int kind, int nlists, int max_len, bool with_nulls) {
  const Column c = make(rng, kind, nlists, max_len, with_nulls);
  const LfCol col = c.view();
  const int64_t rows = nlists, hi = c.offs.back();
  const int32_t* offs = c.offs.data();
  // the keys: one per list as a key column with NULLs (fixed-width kinds), and one literal — element 0 of a one-element column of its own
  Column keys;
  keys.kind = kind;
  keys.with_nulls = true;
  for (int l = 0; l < nlists; l++) {
    keys.is_null.push_back(rng() % 6 == 0);
    push_value(rng, keys);
  }
  if (nlists == 0) {
    keys.is_null.push_back(false);
    push_value(rng, keys);
  }
  keys.build();
  LpKey lit;
  memset(&lit, 0, sizeof lit);
  const LfCol kc = keys.view();
  std::vector<uint8_t> lit_bytes(keys.text[0].begin(), keys.text[0].end());      // exactly the key's bytes
  lit.key = lf_key(kc, 0);
  lit.bytes = lit_bytes.data();
  lit.len = (int32_t)lit_bytes.size();
  LpKey by_col;
  memset(&by_col, 0, sizeof by_col);
  by_col.col = kc;
  by_col.use_col = 1;
  const int64_t starts[] = {1, 2, 3, -1, -2, -3, 64, -64, 257, INT64_MAX, INT64_MIN};
  const int64_t lengths[] = {0, 1, 2, 3, 100, INT64_MAX};
  const int64_t start = starts[rng() % 11], length = lengths[rng() % 6];
  std::vector<uint32_t> rev((size_t)hi, 0xffffffffu);
  for (int64_t e = 0; e < hi; e++) {
    const int64_t row = lf_list_of(offs, rows, e);
    const int64_t first = offs[row], end = offs[row + 1];
    expect(first <= e && e < end, "lf_list_of", kind, e);
    const bool null = c.is_null[(size_t)e];
    // remove by the literal
    const bool eq_lit = !null && (kind == LF_STR ? c.text[(size_t)e] == keys.text[0] : c.num[(size_t)e] == keys.num[0]);
    expect(lp_keep(LP_REMOVE, col, row, first, end, e, lit, 0, 0) == !eq_lit, "remove by a literal", kind, e);
    if (kind != LF_STR) {
      const bool knull = keys.is_null[(size_t)row];
      const bool want = knull ? false : !(!null && c.num[(size_t)e] == keys.num[(size_t)row]);
      expect(lp_keep(LP_REMOVE, col, row, first, end, e, by_col, 0, 0) == want, "remove by a key column", kind, e);
    }
    expect(lp_keep(LP_COMPACT, col, row, first, end, e, lit, 0, 0) == !null, "compact", kind, e);
    {
      const int64_t n = end - first, pos = e - first;
      bool want = false;
      if (start > 0 ? start - 1 < n : start >= -n) {      // (a start before the beginning, or past the end, keeps nothing)
        const int64_t z = start > 0 ? start - 1 : n + start;
        want = pos >= z && (length > n || pos < z + length);
      }
      expect(lp_keep(LP_SLICE, col, row, first, end, e, lit, start, length) == want, "slice", kind, e);
    }
    const int64_t slot = lp_reverse_slot(first, end, e);
    expect(slot >= first && slot < end, "reverse: the slot lies in the list", kind, e);
    if (slot >= 0 && slot < hi) rev[(size_t)slot] = (uint32_t)e;
  }
  for (int64_t r = 0; r < rows; r++)
    for (int64_t j = offs[r]; j < offs[r + 1]; j++) expect(rev[(size_t)j] == (uint32_t)(offs[r] + offs[r + 1] - 1 - j), "reverse", kind, j);
  if (kind != LF_STR) return;
  // join, in the kernels' steps, with and without a replacement
  for (int with_rep = 0; with_rep < 2; with_rep++) {
    const std::string dtext = rng() % 3 == 0 ? "" : rng() % 2 ? "," : ", \xe2\x86\x92 ", rtext = rng() % 3 == 0 ? "" : "NULL";
    const std::vector<uint8_t> d(dtext.begin(), dtext.end()), rp(rtext.begin(), rtext.end());
    const int32_t dn = (int32_t)d.size(), rn = with_rep ? (int32_t)rp.size() : 0;
    std::vector<uint32_t> flag((size_t)hi), len((size_t)hi, 0u);
    std::vector<int32_t> F((size_t)hi + 1, 0), P((size_t)hi + 1, 0);
    for (int64_t e = 0; e < hi; e++) flag[(size_t)e] = lp_is_piece(col, e, with_rep != 0) ? 1u : 0u;
    for (int64_t e = 0; e < hi; e++) F[(size_t)e + 1] = F[(size_t)e] + (int32_t)flag[(size_t)e];
    for (int64_t e = 0; e < hi; e++)
      if (flag[(size_t)e]) len[(size_t)e] = lp_piece_len(col, e, F[(size_t)e] == F[(size_t)offs[lf_list_of(offs, rows, e)]], dn, rn);
    for (int64_t e = 0; e < hi; e++) P[(size_t)e + 1] = P[(size_t)e] + (int32_t)len[(size_t)e];
    std::vector<uint8_t> bytes((size_t)P[(size_t)hi]);
    for (int64_t e = 0; e < hi; e++)
      if (flag[(size_t)e]) lp_piece_write(col, e, F[(size_t)e] == F[(size_t)offs[lf_list_of(offs, rows, e)]], d.data(), dn, rp.data(), rn, bytes.data() + P[(size_t)e]);
    for (int64_t r = 0; r < rows; r++) {
      std::string want;
      bool any = false;
      for (int64_t j = offs[r]; j < offs[r + 1]; j++) {
        if (c.is_null[(size_t)j] && !with_rep) continue;
        if (any) want += dtext;
        want += c.is_null[(size_t)j] ? rtext : c.text[(size_t)j];
        any = true;
      }
      const int32_t lo = P[(size_t)offs[r]], end = P[(size_t)offs[r + 1]];      // what list_offsets_kernel reads
      expect(std::string(bytes.begin() + lo, bytes.begin() + end) == want, with_rep ? "join with a replacement" : "join", kind, r);
    }
  }
}

}  // namespace

int main() {
  std::mt19937_64 rng(20261021);
  const int kinds[] = {LF_BOOL, LF_I8, LF_I16, LF_I32, LF_I64, LF_I128, LF_STR};
  for (int kind : kinds) {
    for (int round = 0; round < 40; round++) check_kind(rng, kind, 1 + (int)(rng() % 40), round % 8 == 0 ? 300 : 7, round % 2 == 0);
    check_kind(rng, kind, 0, 5, true);
    check_kind(rng, kind, 3, 0, true);      // only empty lists
    check_kind(rng, kind, 2, 5000, true);
  }
  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  printf("ok\n");
  return 0;
}
