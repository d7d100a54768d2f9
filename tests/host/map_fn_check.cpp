// csrc/device/map_fn.hpp — the entry search that the fused kernels run for map_extract, and utf8_eq_rows — over random maps against a std::find_if
// restatement.  Every buffer is a vector of exactly the bytes Arrow would hand over, so a read past an end is an AddressSanitizer report; a NULL map's offsets
// span entries whose key rows lie far outside the key column, so reading an entry before the validity bit is one too.  Built with
// -fsanitize=address,undefined by tests/test_map_fn_cpu.py and run on the CPU; prints "ok" and exits 0 when every answer was right.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "device/map_fn.hpp"

namespace {

int failures = 0;
void fail(const char* what, int kind, long long row) {
  if (failures++ < 10) fprintf(stderr, "FAIL %s kind %d row %lld\n", what, kind, row);
}

enum Kind { K_BOOL, K_I8, K_I16, K_I32, K_I64, K_DEC64, K_DEC128, K_STR };

const char* const kWords[] = {"", "a", "ab", "abcdefgh", "abcdefghi", "abcdefghj", "abcdefgh\x01", "\xe6\x97\xa5", "\xe6\x97\xa5\xe6\x9c\xac", "\xff", "zzzzzzzzzzzzzzzzzzzz", "zzzzzzzzzzzzzzzzzzzy"};
constexpr int kNumWords = 12;

struct Keys {      // a key column (or a column of wanted keys): the values, and their Arrow buffers
  int kind = K_I64;
  std::vector<__int128> num;
  std::vector<std::string> text;
  std::vector<uint8_t> data, aux;
  void add(std::mt19937_64& rng) {
    if (kind == K_STR) {
      std::string s = kWords[rng() % kNumWords];
      if (rng() % 7 == 0) s.push_back('\0');
      text.push_back(s);
      num.push_back(0);
      return;
    }
    __int128 v = (__int128)(int64_t)(rng() % 5) - 2;
    const int bits = kind == K_I8 ? 8 : kind == K_I16 ? 16 : kind == K_I32 ? 32 : kind == K_DEC128 ? 127 : 64;
    const int pick = (int)(rng() % 9);
    if (kind == K_BOOL) v = (int)(rng() & 1);
    else if (pick == 0) v = -((__int128)1 << (bits - 1));
    else if (pick == 1) v = ((__int128)1 << (bits - 1)) - 1;
    else if (pick == 2 && kind == K_DEC128) v = ((__int128)1 << 64) + (int64_t)(rng() % 3);      // equal low words, different high words
    num.push_back(v);
    text.emplace_back();
  }
  void pack() {
    const size_t n = num.size();
    if (kind == K_STR) {
      data.assign((n + 1) * 4, 0);
      int32_t at = 0;
      for (size_t i = 0; i < n; i++) {
        memcpy(&data[i * 4], &at, 4);
        aux.insert(aux.end(), text[i].begin(), text[i].end());
        at += (int32_t)text[i].size();
      }
      memcpy(&data[n * 4], &at, 4);
      return;
    }
    if (kind == K_BOOL) {
      data.assign((n + 7) / 8, 0);
      for (size_t i = 0; i < n; i++)
        if (num[i]) data[i >> 3] |= (uint8_t)(1u << (i & 7));
      return;
    }
    const size_t w = kind == K_I8 ? 1 : kind == K_I16 ? 2 : kind == K_I32 ? 4 : kind == K_I64 ? 8 : 16;
    data.assign(n * w, 0);
    for (size_t i = 0; i < n; i++) {
      const __int128 v = num[i];      // (little-endian two's complement: Decimal128 of up to 18 digits carries its sign extension in the upper limb)
      memcpy(&data[i * w], &v, w);
    }
  }
  CometCol view() const {
    CometCol c;
    c.data = data.data();
    c.valid = nullptr;
    c.aux = aux.empty() ? nullptr : aux.data();
    c.offset = 0;
    return c;
  }
};

struct Maps {
  std::vector<int32_t> offs;
  std::vector<uint8_t> valid;
  std::vector<bool> is_null;
  Keys keys;
};

// maps of 0 … max_len entries; a NULL map spans up to two entries of its own, as Arrow allows: garbage that may well hold the wanted key
Maps make(std::mt19937_64& rng, int kind, int nmaps, int max_len, bool with_nulls) {
  Maps m;
  m.keys.kind = kind;
  std::vector<int> lens;
  for (int r = 0; r < nmaps; r++) {
    m.is_null.push_back(with_nulls && rng() % 4 == 0);
    lens.push_back(m.is_null.back() ? (int)(rng() % 3) : (int)(rng() % (uint64_t)(max_len + 1)));
    for (int i = 0; i < lens.back(); i++) m.keys.add(rng);
  }
  m.keys.pack();
  m.offs.assign((size_t)nmaps + 1, 0);
  int32_t at = 0;
  for (int r = 0; r < nmaps; r++) {
    m.offs[(size_t)r] = at;
    at += lens[(size_t)r];
  }
  m.offs[(size_t)nmaps] = at;
  if (with_nulls) {
    m.valid.assign(((size_t)nmaps + 7) / 8, 0);
    for (int r = 0; r < nmaps; r++)
      if (!m.is_null[(size_t)r]) m.valid[(size_t)r >> 3] |= (uint8_t)(1u << (r & 7));
  }
  return m;
}

// the restatement: the first entry of row r whose key is wanted key j, -1 for a NULL map whatever its offsets span
long long want_of(const Maps& m, int r, const Keys& wanted, int j) {
  if (m.is_null[(size_t)r]) return -1;
  const int32_t a = m.offs[(size_t)r], b = m.offs[(size_t)r + 1];
  if (m.keys.kind == K_STR) {
    auto it = std::find_if(m.keys.text.begin() + a, m.keys.text.begin() + b, [&](const std::string& s) { return s == wanted.text[(size_t)j]; });
    return it == m.keys.text.begin() + b ? -1 : (long long)(it - m.keys.text.begin());
  }
  auto it = std::find_if(m.keys.num.begin() + a, m.keys.num.begin() + b, [&](__int128 v) { return v == wanted.num[(size_t)j]; });
  return it == m.keys.num.begin() + b ? -1 : (long long)(it - m.keys.num.begin());
}

long long got_of(const CometCol& mc, bool hv, const CometCol& kc, int kind, long long r, const Keys& wanted, const CometCol& wc, int j) {
  const __int128 k = wanted.num[(size_t)j];
  switch (kind) {
    case K_BOOL: return mf_find<MfBool>(mc, hv, kc, r, k != 0);
    case K_I8: return mf_find<MfI8>(mc, hv, kc, r, (int)k);
    case K_I16: return mf_find<MfI16>(mc, hv, kc, r, (int)k);
    case K_I32: return mf_find<MfI32>(mc, hv, kc, r, (int)k);
    case K_I64: return mf_find<MfI64>(mc, hv, kc, r, (long long)k);
    case K_DEC64: return mf_find<MfDec64>(mc, hv, kc, r, (long long)k);
    case K_DEC128: return mf_find<MfDec128>(mc, hv, kc, r, k);
    default: {
      const std::string& s = wanted.text[(size_t)j];
      const long long a = mf_find_lit(mc, hv, kc, r, s.data(), (int)s.size());
      const long long b = mf_find_row(mc, hv, kc, r, wc, j);
      if (a != b) fail("literal and column key disagree", kind, r);
      return a;
    }
  }
}

void check(std::mt19937_64& rng, int kind, int nmaps, int max_len, bool with_nulls) {
  const Maps m = make(rng, kind, nmaps, max_len, with_nulls);
  CometCol mc;
  mc.data = m.offs.data();
  mc.valid = m.valid.empty() ? nullptr : m.valid.data();
  mc.aux = nullptr;
  mc.offset = 0;
  const CometCol kc = m.keys.view();
  // the wanted keys: random ones, and for every map its first and its last key
  Keys wanted;
  wanted.kind = kind == K_DEC64 ? K_I64 : kind;
  std::vector<int> row_of;
  for (int r = 0; r < nmaps; r++) {
    wanted.add(rng);
    row_of.push_back(r);
    const int32_t a = m.offs[(size_t)r], b = m.offs[(size_t)r + 1];
    if (b > a) {      // (a NULL map's garbage keys too: the answer stays -1)
      for (int32_t e : {a, b - 1}) {
        wanted.num.push_back(m.keys.num[(size_t)e]);
        wanted.text.push_back(m.keys.text[(size_t)e]);
        row_of.push_back(r);
      }
    }
  }
  wanted.pack();
  const CometCol wc = wanted.view();
  for (size_t j = 0; j < row_of.size(); j++) {
    const int r = row_of[j];
    if (got_of(mc, with_nulls, kc, kind, r, wanted, wc, (int)j) != want_of(m, r, wanted, (int)j)) fail("mf_find", kind, r);
  }
}

// one NULL map whose offsets span entries that do not exist: the validity bit comes first
void check_null_over_garbage(int kind) {
  std::mt19937_64 rng(99);
  Keys keys, wanted;
  keys.kind = kind;
  wanted.kind = kind == K_DEC64 ? K_I64 : kind;
  keys.add(rng);
  keys.pack();
  wanted.add(rng);
  wanted.pack();
  const std::vector<int32_t> offs = {1000000, 2000000};
  const std::vector<uint8_t> valid = {0};
  CometCol mc;
  mc.data = offs.data();
  mc.valid = valid.data();
  mc.aux = nullptr;
  mc.offset = 0;
  if (got_of(mc, true, keys.view(), kind, 0, wanted, wanted.view(), 0) != -1) fail("a NULL map over garbage offsets", kind, 0);
}

void check_utf8_eq_rows() {
  std::mt19937_64 rng(5);
  Keys a, b;
  a.kind = b.kind = K_STR;
  for (int i = 0; i < 300; i++) { a.add(rng); b.add(rng); }
  a.pack();
  b.pack();
  const CometCol ac = a.view(), bc = b.view();
  for (int i = 0; i < 300; i++)
    for (int j = 0; j < 300; j++) {
      if (utf8_eq_rows(ac, i, bc, j) != (a.text[(size_t)i] == b.text[(size_t)j])) fail("utf8_eq_rows", K_STR, i);
      if (mf_utf8_eq_lit(ac, i, b.text[(size_t)j].data(), (int)b.text[(size_t)j].size()) != (a.text[(size_t)i] == b.text[(size_t)j])) fail("mf_utf8_eq_lit", K_STR, i);
    }
}

}  // namespace

int main() {
  std::mt19937_64 rng(20260101);
  for (int kind = K_BOOL; kind <= K_STR; kind++) {
    for (int trial = 0; trial < 20; trial++) {
      check(rng, kind, 200, 6, true);
      check(rng, kind, 50, 6, false);
    }
    check(rng, kind, 5, 0, true);         // empty maps only
    check(rng, kind, 5, 300, true);       // beyond a wave
    check_null_over_garbage(kind);
  }
  check_utf8_eq_rows();
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  puts("ok");
  return 0;
}
