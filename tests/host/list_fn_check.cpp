// csrc/device/list_fn.hpp — the per-element code of array_sort / array_distinct that list_kernels.hip runs on the device — over random lists against
// std::stable_sort and a plain first-occurrence scan.  Every buffer is a vector of exactly the bytes Arrow would hand over, so a read past an end is an
// AddressSanitizer report.  Built with -fsanitize=address,undefined by tests/test_list_fn_cpu.py and run on the CPU; prints "ok" and exits 0 when every
// answer was right.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "device/list_fn.hpp"

namespace {

struct Column {      // several lists laid end to end, as a list column's element column is
  int kind = LF_I64;
  std::vector<uint8_t> data, aux, valid;
  std::vector<int32_t> offs;                       // the lists' offsets
  std::vector<bool> is_null;
  std::vector<std::string> text;                   // LF_STR: the values
  std::vector<__int128> num;                       // the others
  LfCol view() const {
    LfCol c;
    c.data = data.data();
    c.aux = aux.empty() ? nullptr : aux.data();
    c.valid = valid.empty() ? nullptr : valid.data();
    c.offset = 0;
    c.kind = kind;
    return c;
  }
};

Column make(std::mt19937_64& rng, int kind, int nlists, int max_len, bool with_nulls) {
  static const char* const words[] = {"", "a", "ab", "abcdefgh", "abcdefghi", "abcdefghj", "abcdefgh\x01", "\xe6\x97\xa5", "\xff", "zzzzzzzzzzzzzzzzzzzz", "zzzzzzzzzzzzzzzzzzzy"};
  Column c;
  c.kind = kind;
  c.offs.push_back(0);
  for (int l = 0; l < nlists; l++) {
    const int n = (int)(rng() % (uint64_t)(max_len + 1));
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
        const int bits = kind == LF_BOOL ? 1 : kind == LF_I128 ? 127 : kind * 8;      // (127: ±2^126 shifts without overflow and exceeds 10^38 − 1)
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
  const size_t n = c.is_null.size();
  if (with_nulls) {
    c.valid.assign((n + 7) / 8, 0);
    for (size_t i = 0; i < n; i++)
      if (!c.is_null[i]) c.valid[i >> 3] |= (uint8_t)(1u << (i & 7));
  }
  if (kind == LF_STR) {
    std::vector<int32_t> so(1, 0);
    for (auto& s : c.text) {
      c.aux.insert(c.aux.end(), s.begin(), s.end());
      so.push_back((int32_t)c.aux.size());
    }
    c.data.resize(so.size() * 4);
    memcpy(c.data.data(), so.data(), c.data.size());
  } else if (kind == LF_BOOL) {
    c.data.assign((n + 7) / 8, 0);
    for (size_t i = 0; i < n; i++)
      if (c.num[i]) c.data[i >> 3] |= (uint8_t)(1u << (i & 7));
  } else {
    c.data.resize(n * (size_t)kind);
    for (size_t i = 0; i < n; i++) memcpy(c.data.data() + i * (size_t)kind, &c.num[i], (size_t)kind);      // little endian
  }
  if (c.data.empty()) c.data.resize(1);
  return c;
}

int value_cmp(const Column& c, size_t a, size_t b) {
  if (c.kind == LF_STR) {
    const std::string &x = c.text[a], &y = c.text[b];
    const int d = memcmp(x.data(), y.data(), std::min(x.size(), y.size()));      // unsigned bytes
    return d ? d : x.size() < y.size() ? -1 : x.size() > y.size() ? 1 : 0;
  }
  return c.num[a] < c.num[b] ? -1 : c.num[a] > c.num[b] ? 1 : 0;
}

long check(std::mt19937_64& rng, int kind, int nlists, int max_len, bool with_nulls) {
  const Column c = make(rng, kind, nlists, max_len, with_nulls);
  const LfCol v = c.view();
  long bad = 0;
  for (int l = 0; l < nlists; l++) {
    const int64_t first = c.offs[(size_t)l], end = c.offs[(size_t)l + 1];
    for (int64_t e = first; e < end; e++)
      if (lf_list_of(c.offs.data(), (lf_i64)nlists, e) < 0 || c.offs[(size_t)lf_list_of(c.offs.data(), (lf_i64)nlists, e)] > e ||
          c.offs[(size_t)lf_list_of(c.offs.data(), (lf_i64)nlists, e) + 1] <= e)
        bad++;
    for (int flags = 0; flags < 4; flags++) {
      std::vector<int64_t> want;
      for (int64_t e = first; e < end; e++) want.push_back(e);
      std::stable_sort(want.begin(), want.end(), [&](int64_t a, int64_t b) {
        const bool an = c.is_null[(size_t)a], bn = c.is_null[(size_t)b];
        if (an != bn) return (flags & LF_NULLS_LAST) ? bn : an;
        if (an) return false;
        const int d = value_cmp(c, (size_t)a, (size_t)b);
        return (flags & LF_DESC) ? d > 0 : d < 0;
      });
      std::vector<int64_t> got((size_t)(end - first), -1);
      for (int64_t e = first; e < end; e++) {
        const int64_t r = lf_rank(v, first, end, e, flags);
        if (r < 0 || r >= end - first || got[(size_t)r] != -1) { bad++; continue; }
        got[(size_t)r] = e;
      }
      if (got != want) bad++;
    }
    for (int64_t e = first; e < end; e++) {
      bool keep = true;
      for (int64_t j = first; j < e && keep; j++)
        if (c.is_null[(size_t)j] == c.is_null[(size_t)e] && (c.is_null[(size_t)e] || value_cmp(c, (size_t)j, (size_t)e) == 0)) keep = false;
      if (lf_keep(v, first, e) != keep) bad++;
    }
  }
  return bad;
}

}  // namespace

int main() {
  std::mt19937_64 rng(20240611);
  long bad = 0;
  const int kinds[] = {LF_BOOL, LF_I8, LF_I16, LF_I32, LF_I64, LF_I128, LF_STR};
  for (int kind : kinds)
    for (int nulls = 0; nulls < 2; nulls++) {
      bad += check(rng, kind, 200, 9, nulls != 0);
      bad += check(rng, kind, 3, 130, nulls != 0);
    }
  if (bad) {
    printf("%ld wrong answers\n", bad);
    return 1;
  }
  printf("ok\n");
  return 0;
}
