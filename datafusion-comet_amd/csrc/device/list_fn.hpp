// Per-list sort and de-duplication of a list column's elements: what a chain's DERIVED list columns of kind 4 are computed with (codegen.hpp DerivedCol;
// list_kernels.hip; exec.cpp extend_derived_list_fn).  Spark's SortArray and ArrayDistinct (serde/arrays.scala sends array_sort(arr, 'ASC' | 'DESC',
// 'NULLS FIRST' | 'NULLS LAST') and array_distinct(arr)):
//   sort      the list's elements by (null rank, value, position) — ascending or descending by value, NULL elements first or last as the flags say
//   distinct  the first occurrence of every value stays where it stands; NULL elements count as one value
// Orders: integers, dates, timestamps and decimals by value, Boolean false < true, Utf8 by unsigned bytes with a proper prefix first.
// The code never moves a value: it answers with element ROW NUMBERS (sort: which source row stands in an output slot) or keep flags (distinct), and the
// executor takes the element column by them.  Position as the last criterion makes "before" a strict total order, so an element's rank — the number of
// elements of its list that stand before it — is its output slot, and every result is a pure function of the input.
// Plain C++ over raw Arrow buffers: list_kernels.hip includes it for the device, capi.cpp runs the same source on the host for the CPU tests
// (comet_list_fn_host) and tests/host/list_fn_check.cpp under the sanitizers.
#pragma once
typedef unsigned char lf_u8;
typedef unsigned int lf_u32;
typedef int lf_i32;
typedef unsigned long long lf_u64;
typedef long long lf_i64;
#ifndef LISTFN
#define LISTFN inline
#endif

// how an element is laid out: Boolean bits, little-endian integers of 1 / 2 / 4 / 8 / 16 bytes (Decimal128: 16), Utf8 as int32 offsets + bytes
enum { LF_BOOL = 0, LF_I8 = 1, LF_I16 = 2, LF_I32 = 4, LF_I64 = 8, LF_I128 = 16, LF_STR = 32 };
enum { LF_OP_SORT = 0, LF_OP_DISTINCT = 1 };
enum { LF_DESC = 1, LF_NULLS_LAST = 2 };

// the element column: `data` the values (LF_STR: the int32 offsets), `aux` LF_STR's bytes, `valid` the validity bits or nullptr; `offset` the column's
// Arrow offset — element row e is entry offset + e of data and valid
struct LfCol {
  const void* data;
  const lf_u8* aux;
  const lf_u8* valid;
  lf_i64 offset;
  int kind;
};

// the order-preserving key of an element: two u64 compared (hi, lo) unsigned.  Up to 8 bytes: the sign-flipped value in lo.  16 bytes: the sign-flipped
// upper half, the lower half.  Utf8: hi = the first 8 bytes big-endian, zero-padded — equal prefixes are decided on the bytes (lf_cmp)
struct LfKey {
  lf_u64 hi, lo;
};

LISTFN bool lf_is_null(const LfCol& c, lf_i64 e) {
  if (!c.valid) return false;
  const lf_i64 j = c.offset + e;
  return !((c.valid[j >> 3] >> (j & 7)) & 1);
}

LISTFN LfKey lf_key(const LfCol& c, lf_i64 e) {
  const lf_i64 j = c.offset + e;
  const lf_u64 sign = 1ull << 63;
  LfKey k;
  k.hi = 0;
  k.lo = 0;
  switch (c.kind) {
    case LF_BOOL: k.lo = (((const lf_u8*)c.data)[j >> 3] >> (j & 7)) & 1; break;
    case LF_I8: k.lo = (lf_u64)(lf_i64)((const signed char*)c.data)[j] ^ sign; break;
    case LF_I16: k.lo = (lf_u64)(lf_i64)((const short*)c.data)[j] ^ sign; break;
    case LF_I32: k.lo = (lf_u64)(lf_i64)((const lf_i32*)c.data)[j] ^ sign; break;
    case LF_I64: k.lo = ((const lf_u64*)c.data)[j] ^ sign; break;
    case LF_I128:
      k.lo = ((const lf_u64*)c.data)[2 * j];
      k.hi = ((const lf_u64*)c.data)[2 * j + 1] ^ sign;
      break;
    default: {
      const lf_i32* off = (const lf_i32*)c.data;
      const lf_i32 lo = off[j], n = off[j + 1] - lo;
      for (lf_i32 b = 0; b < 8; b++) k.hi = (k.hi << 8) | (b < n ? (lf_u64)c.aux[(lf_i64)lo + b] : 0ull);
    }
  }
  return k;
}

// the values of elements a and b (neither NULL), whose keys are ka and kb: < 0, 0, > 0
LISTFN int lf_cmp(const LfCol& c, const LfKey& ka, lf_i64 a, const LfKey& kb, lf_i64 b) {
  if (ka.hi != kb.hi) return ka.hi < kb.hi ? -1 : 1;
  if (c.kind != LF_STR) return ka.lo == kb.lo ? 0 : ka.lo < kb.lo ? -1 : 1;
  // equal 8-byte prefixes (zero padding included: "a" and "a\0" meet here): the bytes decide, then the lengths
  const lf_i32* off = (const lf_i32*)c.data;
  const lf_i32 alo = off[c.offset + a], an = off[c.offset + a + 1] - alo, blo = off[c.offset + b], bn = off[c.offset + b + 1] - blo;
  const lf_i32 m = an < bn ? an : bn;
  for (lf_i32 i = 0; i < m; i++) {
    const lf_u8 x = c.aux[(lf_i64)alo + i], y = c.aux[(lf_i64)blo + i];
    if (x != y) return x < y ? -1 : 1;
  }
  return an == bn ? 0 : an < bn ? -1 : 1;
}

// 1 for the elements that sort behind the others by NULL-ness alone
LISTFN int lf_null_rank(bool is_null, int flags) { return is_null == ((flags & LF_NULLS_LAST) != 0) ? 1 : 0; }

// does element a stand before element b in the sorted list?  (null rank, value in the flags' direction, position)
LISTFN bool lf_before(const LfCol& c, int flags, bool a_null, const LfKey& ka, lf_i64 a, bool b_null, const LfKey& kb, lf_i64 b) {
  const int ra = lf_null_rank(a_null, flags), rb = lf_null_rank(b_null, flags);
  if (ra != rb) return ra < rb;
  if (!a_null) {
    const int d = lf_cmp(c, ka, a, kb, b);
    if (d != 0) return (flags & LF_DESC) ? d > 0 : d < 0;
  }
  return a < b;
}

// the number of elements of the list [first, end) that stand before element e of it: e's slot in the sorted list
LISTFN lf_i64 lf_rank(const LfCol& c, lf_i64 first, lf_i64 end, lf_i64 e, int flags) {
  const bool e_null = lf_is_null(c, e);
  LfKey ke;
  ke.hi = ke.lo = 0;
  if (!e_null) ke = lf_key(c, e);
  lf_i64 before = 0;
  for (lf_i64 j = first; j < end; j++) {
    if (j == e) continue;
    const bool j_null = lf_is_null(c, j);
    LfKey kj;
    kj.hi = kj.lo = 0;
    if (!j_null) kj = lf_key(c, j);
    before += lf_before(c, flags, j_null, kj, j, e_null, ke, e) ? 1 : 0;
  }
  return before;
}

// does element e of the list that starts at `first` stay in the distinct list?  No earlier element has its NULL-ness and value
LISTFN bool lf_keep(const LfCol& c, lf_i64 first, lf_i64 e) {
  const bool e_null = lf_is_null(c, e);
  LfKey ke;
  ke.hi = ke.lo = 0;
  if (!e_null) ke = lf_key(c, e);
  for (lf_i64 j = first; j < e; j++) {
    const bool j_null = lf_is_null(c, j);
    if (j_null != e_null) continue;
    if (e_null) return false;
    const LfKey kj = lf_key(c, j);
    if (lf_cmp(c, kj, j, ke, e) == 0) return false;
  }
  return true;
}

// the list that holds element row e: the last row i of offs[0 … rows] with offs[i] <= e (the caller knows offs[0] <= e < offs[rows]); empty and NULL lists
// repeat an offset and are passed over
template <class P>
LISTFN lf_i64 lf_list_of(P offs, lf_i64 rows, lf_i64 e) {
  lf_i64 lo = 0, hi = rows;      // offs[lo] <= e < offs[hi]
  while (hi - lo > 1) {
    const lf_i64 mid = lo + (hi - lo) / 2;
    if ((lf_i64)offs[mid] <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}
