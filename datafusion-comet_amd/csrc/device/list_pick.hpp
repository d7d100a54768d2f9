// The functions of ONE list that give back some of its elements, or its elements as one string: what a chain's DERIVED columns of kind 7 are computed with
// (codegen.hpp DerivedCol; list_pick_kernels.hip; exec.cpp extend_derived_list_pick).  Spark's ArrayRemove, array_compact, Slice, Reverse of an array and
// ArrayJoin (serde/arrays.scala sends array_remove_all(arr, key), array_compact(arr), spark_array_slice(arr, start, length), array_reverse(arr) and
// array_to_string(arr, delimiter[, nullReplacement])):
//   remove    the list without its non-NULL elements equal to the key; NULL elements stay (a NULL key makes the ROW NULL: the caller's business)
//   compact   the list without its NULL elements
//   slice     z = start - 1 for start > 0, start + n for start < 0; nothing when z < 0, z >= n or length = 0, else the min(length, n - z) elements from z
//   reverse   the elements in reverse position order
//   join      the non-NULL elements — or, with a replacement, every element, a NULL one as the replacement — with the delimiter between them
// Every answer is O(1) per element once its list is known (lf_list_of), so a list of 5 000 elements takes the path of one of 3.  Like list_fn.hpp the code
// never moves a value of a list result: it answers with keep flags or element ROW NUMBERS and the executor takes the element column by them; only join writes
// bytes.  Plain C++ over raw Arrow buffers: list_pick_kernels.hip includes it for the device, capi.cpp runs the same source on the host for the CPU tests
// (comet_list_pick_host) and tests/host/list_pick_check.cpp under the sanitizers.
#pragma once
#include "list_fn.hpp"

enum { LP_REMOVE = 0, LP_COMPACT = 1, LP_SLICE = 2, LP_REVERSE = 3, LP_JOIN = 4 };

// remove's key.  A literal: `key` as lf_key gives it for an element of the same value (Utf8: the first 8 bytes) and for Utf8 its `len` bytes at `bytes`.
// A column of the chain (fixed-width elements only): `col`, indexed by the LIST row, with use_col set — `key`, `bytes` and `len` are not read then
struct LpKey {
  LfKey key;
  const lf_u8* bytes;
  lf_i32 len;
  LfCol col;
  int use_col;
};

// is element e (not NULL) equal to the literal key?
LISTFN bool lp_eq_lit(const LfCol& c, lf_i64 e, const LpKey& k) {
  const LfKey ke = lf_key(c, e);
  if (ke.hi != k.key.hi) return false;
  if (c.kind != LF_STR) return ke.lo == k.key.lo;
  const lf_i32* off = (const lf_i32*)c.data;
  const lf_i32 lo = off[c.offset + e], n = off[c.offset + e + 1] - lo;
  if (n != k.len) return false;
  for (lf_i32 i = 8; i < n; i++)      // (the first 8 bytes are the keys' hi words, and the lengths are equal)
    if (c.aux[(lf_i64)lo + i] != k.bytes[i]) return false;
  return true;
}

// remove: does element e of list row `row` stay?  Not (non-NULL and equal to the key); under a NULL key of a key column nothing stays (the row is NULL)
LISTFN bool lp_keep_remove(const LfCol& c, lf_i64 row, lf_i64 e, const LpKey& k) {
  if (k.use_col) {
    if (lf_is_null(k.col, row)) return false;
    if (lf_is_null(c, e)) return true;
    const LfKey ke = lf_key(c, e), kk = lf_key(k.col, row);
    return !(ke.hi == kk.hi && ke.lo == kk.lo);
  }
  if (lf_is_null(c, e)) return true;
  return !lp_eq_lit(c, e, k);
}

// slice: does the element at position pos of a list of n elements stay?  (start != 0 and length >= 0: the plan is refused otherwise)
LISTFN bool lp_keep_slice(lf_i64 n, lf_i64 pos, lf_i64 start, lf_i64 length) {
  const lf_i64 z = start > 0 ? start - 1 : start + n;
  if (z < 0 || z >= n || length <= 0) return false;
  const lf_i64 take = length < n - z ? length : n - z;
  return pos >= z && pos - z < take;
}

// the keep flag of element e of the list [first, end) of row `row`, for the three operations that drop elements
LISTFN bool lp_keep(int op, const LfCol& c, lf_i64 row, lf_i64 first, lf_i64 end, lf_i64 e, const LpKey& k, lf_i64 start, lf_i64 length) {
  if (op == LP_REMOVE) return lp_keep_remove(c, row, e, k);
  if (op == LP_COMPACT) return !lf_is_null(c, e);
  return lp_keep_slice(end - first, e - first, start, length);
}

// reverse: the slot of the list [first, end) that element e moves to — a permutation inside the list
LISTFN lf_i64 lp_reverse_slot(lf_i64 first, lf_i64 end, lf_i64 e) { return first + (end - 1 - e); }

// join: is element e a piece of the result?  A non-NULL element, or any element when a replacement is given
LISTFN bool lp_is_piece(const LfCol& c, lf_i64 e, bool has_rep) { return has_rep || !lf_is_null(c, e); }

// … the bytes it brings: the element's or the replacement's, and the delimiter's unless it is its list's first piece
LISTFN lf_u32 lp_piece_len(const LfCol& c, lf_i64 e, bool first_piece, lf_i32 dn, lf_i32 rn) {
  lf_i32 n = rn;
  if (!lf_is_null(c, e)) {
    const lf_i32* off = (const lf_i32*)c.data;
    n = off[c.offset + e + 1] - off[c.offset + e];
  }
  return (lf_u32)n + (first_piece ? 0u : (lf_u32)dn);
}

// … and writes them at dst
LISTFN void lp_piece_write(const LfCol& c, lf_i64 e, bool first_piece, const lf_u8* d, lf_i32 dn, const lf_u8* r, lf_i32 rn, lf_u8* dst) {
  if (!first_piece) {
    for (lf_i32 i = 0; i < dn; i++) dst[i] = d[i];
    dst += dn;
  }
  if (lf_is_null(c, e)) {
    for (lf_i32 i = 0; i < rn; i++) dst[i] = r[i];
    return;
  }
  const lf_i32* off = (const lf_i32*)c.data;
  const lf_i32 lo = off[c.offset + e], n = off[c.offset + e + 1] - lo;
  for (lf_i32 i = 0; i < n; i++) dst[i] = c.aux[(lf_i64)lo + i];
}
