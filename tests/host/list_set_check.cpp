// csrc/device/list_set.hpp — the per-element code of array_union / array_intersect / array_except / arrays_overlap that list_set_kernels.hip runs on the
// device — over random pairs of list columns against a naive O(n·m) check: the find in a sorted list, the member flags, the overlap row function, and the
// concatenation's lengths, source rows and bits.  Every buffer is a vector of exactly the bytes Arrow would hand over, so a read past an end is an
// AddressSanitizer report.  Built with -fsanitize=address,undefined by tests/test_list_set_cpu.py and run on the CPU; prints "ok" and exits 0 when every
// answer was right.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "device/list_set.hpp"

namespace {

struct Column {      // several lists laid end to end, as a list column's element column is
  int kind = LF_I64;
  bool with_nulls = false;
  std::vector<uint8_t> data, aux, valid, row_bits;   // row_bits: the LISTS' validity (empty: every list is valid)
  std::vector<int32_t> offs;                         // the lists' offsets
  std::vector<bool> is_null;
  std::vector<std::string> text;                     // LF_STR: the values
  std::vector<__int128> num;                         // the others
  LfCol view() const {
    LfCol c;
    c.data = data.data();
    c.aux = aux.empty() ? nullptr : aux.data();
    c.valid = valid.empty() ? nullptr : valid.data();
    c.offset = 0;
    c.kind = kind;
    return c;
  }
  void build() {      // the Arrow buffers of is_null / text / num
    const size_t n = is_null.size();
    data.clear();
    aux.clear();
    valid.clear();
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
};

Column make(std::mt19937_64& rng, int kind, int nlists, int max_len, bool with_nulls, bool null_lists) {
  static const char* const words[] = {"", "a", "ab", "abcdefgh", "abcdefghi", "abcdefghj", "abcdefgh\x01", "\xe6\x97\xa5", "\xff", "zzzzzzzzzzzzzzzzzzzz", "zzzzzzzzzzzzzzzzzzzy"};
  Column c;
  c.kind = kind;
  c.with_nulls = with_nulls;
  c.offs.push_back(0);
  if (null_lists) c.row_bits.assign(((size_t)nlists + 7) / 8, 0);
  for (int l = 0; l < nlists; l++) {
    const int n = (int)(rng() % (uint64_t)(max_len + 1));
    if (null_lists && rng() % 6 != 0) c.row_bits[(size_t)l >> 3] |= (uint8_t)(1u << (l & 7));      // (a NULL list may span elements: nothing may read them)
    for (int i = 0; i < n; i++) {
      c.is_null.push_back(with_nulls && rng() % 5 == 0);
      if (kind == LF_STR) {
        std::string s = words[rng() % 11];
        if (rng() % 7 == 0) s.push_back('\0');      // a value that is another plus a zero byte: equal zero-padded prefixes
        c.text.push_back(s);
        c.num.push_back(0);
      } else {
        __int128 v = (__int128)(int64_t)(rng() % 7) - 3;
        const int pick = (int)(rng() % 9);
        const int bits = kind == LF_BOOL ? 1 : kind == LF_I128 ? 127 : kind * 8;
        if (kind == LF_BOOL) v = (int)(rng() & 1);
        else if (pick == 0) v = -((__int128)1 << (bits - 1));
        else if (pick == 1) v = ((__int128)1 << (bits - 1)) - 1;
        else if (pick == 2 && kind == LF_I128) v = ((__int128)1 << 64) + (int64_t)(rng() % 3);
        c.num.push_back(v);
        c.text.emplace_back();
      }
    }
    c.offs.push_back((int32_t)c.is_null.size());
  }
  c.build();
  return c;
}

int value_cmp(const Column& x, size_t a, const Column& y, size_t b) {
  if (x.kind == LF_STR) {
    const std::string &s = x.text[a], &t = y.text[b];
    const int d = memcmp(s.data(), t.data(), std::min(s.size(), t.size()));      // unsigned bytes
    return d ? d : s.size() < t.size() ? -1 : s.size() > t.size() ? 1 : 0;
  }
  return x.num[a] < y.num[b] ? -1 : x.num[a] > y.num[b] ? 1 : 0;
}

// every list of c sorted ascending with its NULL elements first, as a column of its own (what array_sort(c, 'ASC', 'NULLS FIRST') delivers)
Column sorted_lists(const Column& c) {
  Column s;
  s.kind = c.kind;
  s.with_nulls = c.with_nulls;
  s.offs = c.offs;
  s.row_bits = c.row_bits;
  for (size_t l = 0; l + 1 < c.offs.size(); l++) {
    std::vector<size_t> idx;
    for (int32_t e = c.offs[l]; e < c.offs[l + 1]; e++) idx.push_back((size_t)e);
    std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) {
      if (c.is_null[a] != c.is_null[b]) return (bool)c.is_null[a];
      return !c.is_null[a] && value_cmp(c, a, c, b) < 0;
    });
    for (size_t e : idx) {
      s.is_null.push_back(c.is_null[e]);
      s.text.push_back(c.text[e]);
      s.num.push_back(c.num[e]);
    }
  }
  s.build();
  return s;
}

bool naive_has(const Column& a, size_t e, const Column& b, int64_t first, int64_t end) {
  for (int64_t j = first; j < end; j++) {
    if (a.is_null[e] != b.is_null[(size_t)j]) continue;
    if (a.is_null[e] || value_cmp(a, e, b, (size_t)j) == 0) return true;
  }
  return false;
}

long check(std::mt19937_64& rng, int kind, int nlists, int max_len, bool nulls_a, bool nulls_b, bool null_lists) {
  const Column a = make(rng, kind, nlists, max_len, nulls_a, null_lists), b = make(rng, kind, nlists, max_len, nulls_b, null_lists && rng() % 2 == 0);
  const Column bs = sorted_lists(b);
  const LfCol va = a.view(), vb = bs.view();
  const lf_u8* ra = a.row_bits.empty() ? nullptr : a.row_bits.data();
  const lf_u8* rb = b.row_bits.empty() ? nullptr : b.row_bits.data();
  const lf_i64 hi_a = a.offs.back(), hi_b = b.offs.back();
  long bad = 0;
  std::vector<lf_u32> hits((size_t)hi_a + 1, 7u);
  std::vector<lf_u32> lens;
  for (int l = 0; l < nlists; l++) {
    const int64_t af = a.offs[(size_t)l], ae = a.offs[(size_t)l + 1], bf = b.offs[(size_t)l], be = b.offs[(size_t)l + 1];
    const bool row_valid = ls_bit(ra, l) && ls_bit(rb, l);
    bool any_hit = false, a_null = false, b_null = false;
    for (int64_t j = bf; j < be; j++) b_null |= (bool)b.is_null[(size_t)j];
    for (int64_t e = af; e < ae; e++) {
      const bool has = naive_has(a, (size_t)e, bs, bf, be);
      if (lf_find(va, e, vb, bf, be) != has) bad++;
      for (int want = 0; want < 2; want++)
        if (lf_member(va, e, vb, bf, be, ra, rb, l, want != 0, false) != (row_valid && has == (want != 0) ? 1u : 0u)) bad++;
      const bool hit = row_valid && !a.is_null[(size_t)e] && has;
      hits[(size_t)e] = lf_member(va, e, vb, bf, be, ra, rb, l, true, true);
      if (hits[(size_t)e] != (hit ? 1u : 0u)) bad++;
      any_hit |= hit;
      a_null |= (bool)a.is_null[(size_t)e];
    }
    const int want = !row_valid ? LS_NULL : (af == ae || bf == be) ? LS_FALSE : any_hit ? LS_TRUE : (a_null || b_null) ? LS_NULL : LS_FALSE;
    if (lf_overlap_row(hits.data(), va, af, ae, vb, bf, be, row_valid) != want) bad++;
    lens.push_back(lf_concat_len(a.offs.data(), b.offs.data(), ra, rb, l));
    if (lens.back() != (row_valid ? (lf_u32)((ae - af) + (be - bf)) : 0u)) bad++;
  }
  // the concatenation: offsets from the lengths, then every output element's source row in a's elements followed by b's
  std::vector<int32_t> out(1, 0);
  for (lf_u32 n : lens) out.push_back(out.back() + (int32_t)n);
  lf_i64 k = 0;
  for (int l = 0; l < nlists; l++) {
    if (lens[(size_t)l] == 0) continue;
    for (int32_t e = a.offs[(size_t)l]; e < a.offs[(size_t)l + 1]; e++, k++)
      if (lf_concat_src(a.offs.data(), b.offs.data(), (const int32_t*)out.data(), (lf_i64)nlists, hi_a, k) != e) bad++;
    for (int32_t e = b.offs[(size_t)l]; e < b.offs[(size_t)l + 1]; e++, k++)
      if (lf_concat_src(a.offs.data(), b.offs.data(), (const int32_t*)out.data(), (lf_i64)nlists, hi_a, k) != hi_a + e) bad++;
  }
  if (k != out.back()) bad++;
  // the two validity bitmaps laid end to end, either of which may be absent
  const Column ub = b;
  const lf_u8* xa = a.valid.empty() ? nullptr : a.valid.data();
  const lf_u8* xb = ub.valid.empty() ? nullptr : ub.valid.data();
  for (lf_i64 i = 0; i < hi_a + hi_b; i++)
    if (ls_concat_bit(xa, hi_a, xb, i) != (i < hi_a ? !a.is_null[(size_t)i] : !ub.is_null[(size_t)(i - hi_a)])) bad++;
  return bad;
}

}  // namespace

int main() {
  std::mt19937_64 rng(20240923);
  long bad = 0;
  const int kinds[] = {LF_BOOL, LF_I8, LF_I16, LF_I32, LF_I64, LF_I128, LF_STR};
  for (int kind : kinds)
    for (int nulls = 0; nulls < 4; nulls++) {
      bad += check(rng, kind, 200, 9, (nulls & 1) != 0, (nulls & 2) != 0, nulls == 3);
      bad += check(rng, kind, 3, 130, (nulls & 1) != 0, (nulls & 2) != 0, false);
    }
  if (bad) {
    printf("%ld wrong answers\n", bad);
    return 1;
  }
  printf("ok\n");
  return 0;
}
