// The set functions over TWO list columns: what a chain's DERIVED columns of kind 6 are computed with (codegen.hpp DerivedCol; list_set_kernels.hip; exec.cpp
// extend_derived_list_set).  Spark's ArrayUnion, ArrayIntersect, ArrayExcept and ArraysOverlap (serde/arrays.scala sends array_union(a, b), array_intersect(a, b),
// array_except(a, b) and spark_arrays_overlap(a, b)):
//   union      distinct(a ++ b): first occurrences, a's before b's
//   intersect  the distinct elements of a, in a's order, that occur in b
//   except     the distinct elements of a, in a's order, that do not occur in b
//   overlap    true when a non-NULL value stands in both; else NULL when either side holds a NULL element and neither is empty; else false
// NULL elements count as one value in the first three; every result is NULL where either list is.  Order and equality are list_fn.hpp's, here across two element
// columns with buffers of their own.  Membership is a binary search of the OTHER side sorted ascending with NULLs first (what array_sort(b, 'ASC', 'NULLS FIRST')
// delivers), so the work per probe element is O(log) in the list's length and no list is too long.  The code moves no value: it answers with flags, with a
// three-valued code per row (overlap) or with source row numbers (the concatenation), and the executor takes the element columns by them.
// Plain C++ over raw Arrow buffers, as list_fn.hpp: list_set_kernels.hip includes it for the device, capi.cpp runs the same source on the host
// (comet_list_set_host) and tests/host/list_set_check.cpp under the sanitizers.
#pragma once
#include "list_fn.hpp"

enum { LS_UNION = 0, LS_INTERSECT = 1, LS_EXCEPT = 2, LS_OVERLAP = 3 };
enum { LS_FALSE = 0, LS_TRUE = 1, LS_NULL = 2 };      // what lf_overlap_row answers

// a validity bit of a bitmap that may be absent (absent: every row is valid)
LISTFN bool ls_bit(const lf_u8* bits, lf_i64 i) { return !bits || ((bits[i >> 3] >> (i & 7)) & 1); }

// the values of element a of column ca and element b of column cb (neither NULL, both columns of one kind), whose keys are ka and kb: < 0, 0, > 0.
// lf_cmp is the case ca == cb
LISTFN int lf_cmp2(const LfCol& ca, const LfKey& ka, lf_i64 a, const LfCol& cb, const LfKey& kb, lf_i64 b) {
  if (ka.hi != kb.hi) return ka.hi < kb.hi ? -1 : 1;
  if (ca.kind != LF_STR) return ka.lo == kb.lo ? 0 : ka.lo < kb.lo ? -1 : 1;
  const lf_i32 *offa = (const lf_i32*)ca.data, *offb = (const lf_i32*)cb.data;
  const lf_i32 alo = offa[ca.offset + a], an = offa[ca.offset + a + 1] - alo, blo = offb[cb.offset + b], bn = offb[cb.offset + b + 1] - blo;
  const lf_i32 m = an < bn ? an : bn;
  for (lf_i32 i = 0; i < m; i++) {
    const lf_u8 x = ca.aux[(lf_i64)alo + i], y = cb.aux[(lf_i64)blo + i];
    if (x != y) return x < y ? -1 : 1;
  }
  return an == bn ? 0 : an < bn ? -1 : 1;
}

// does an element equal to probe element e of column ca stand in the list [first, end) of column cb?  That list is sorted ascending with its NULL elements
// first.  A NULL probe is found if and only if the list's first element is NULL; a value is looked for among the non-NULL elements only
LISTFN bool lf_find(const LfCol& ca, lf_i64 e, const LfCol& cb, lf_i64 first, lf_i64 end) {
  if (first >= end) return false;
  if (lf_is_null(ca, e)) return lf_is_null(cb, first);
  // the first non-NULL element: NULLs stand first, so "is NULL" is monotone over the list
  lf_i64 lo = first, hi = end;      // elements before lo are NULL, elements from hi on are not
  while (lo < hi) {
    const lf_i64 mid = lo + (hi - lo) / 2;
    if (lf_is_null(cb, mid)) lo = mid + 1;
    else hi = mid;
  }
  const LfKey ke = lf_key(ca, e);
  hi = end;                         // elements before lo are less than the probe, elements from hi on are greater
  while (lo < hi) {
    const lf_i64 mid = lo + (hi - lo) / 2;
    const LfKey km = lf_key(cb, mid);
    const int d = lf_cmp2(ca, ke, e, cb, km, mid);
    if (d == 0) return true;
    if (d < 0) hi = mid;
    else lo = mid + 1;
  }
  return false;
}

// the member flag of probe element e, which belongs to list `row` of a: 1 when (it is found in b's sorted list of that row) == want, else 0.  A row that is
// NULL on either side keeps nothing.  values_only (overlap's hits): a NULL probe counts as not found
LISTFN lf_u32 lf_member(const LfCol& ca, lf_i64 e, const LfCol& cb, lf_i64 b_first, lf_i64 b_end, const lf_u8* a_rows, const lf_u8* b_rows, lf_i64 row, bool want, bool values_only) {
  if (!ls_bit(a_rows, row) || !ls_bit(b_rows, row)) return 0u;
  if (values_only && lf_is_null(ca, e)) return 0u;
  return lf_find(ca, e, cb, b_first, b_end) == want ? 1u : 0u;
}

// arrays_overlap of one row: hits[e] is set for the non-NULL elements e of a's list [a_first, a_end) that stand in b's; cb is b SORTED (NULLs first), so its
// list [b_first, b_end) holds a NULL element exactly when its first element is one.  The lane walks a's list once (flags and validity bits)
LISTFN int lf_overlap_row(const lf_u32* hits, const LfCol& ca, lf_i64 a_first, lf_i64 a_end, const LfCol& cb, lf_i64 b_first, lf_i64 b_end, bool row_valid) {
  if (!row_valid) return LS_NULL;
  if (a_first >= a_end || b_first >= b_end) return LS_FALSE;      // an empty side: false, even beside [NULL]
  bool a_null = false;
  for (lf_i64 e = a_first; e < a_end; e++) {
    if (hits[e]) return LS_TRUE;
    a_null |= lf_is_null(ca, e);
  }
  return (a_null || lf_is_null(cb, b_first)) ? LS_NULL : LS_FALSE;
}

// the length of row `row` of a ++ b: both lists' lengths, 0 where either list is NULL
template <class P>
LISTFN lf_u32 lf_concat_len(P offs_a, P offs_b, const lf_u8* a_rows, const lf_u8* b_rows, lf_i64 row) {
  if (!ls_bit(a_rows, row) || !ls_bit(b_rows, row)) return 0u;
  return (lf_u32)(offs_a[row + 1] - offs_a[row]) + (lf_u32)(offs_b[row + 1] - offs_b[row]);
}

// the source of output element k of a ++ b, as a row number of the two element columns laid end to end (a's hi_a rows, then b's): offs_out are the
// concatenation's offsets (rows + 1 of them; the caller knows offs_out[0] <= k < offs_out[rows])
template <class P>
LISTFN lf_i64 lf_concat_src(P offs_a, P offs_b, P offs_out, lf_i64 rows, lf_i64 hi_a, lf_i64 k) {
  const lf_i64 row = lf_list_of(offs_out, rows, k);
  const lf_i64 j = k - (lf_i64)offs_out[row], la = (lf_i64)offs_a[row + 1] - (lf_i64)offs_a[row];
  return j < la ? (lf_i64)offs_a[row] + j : hi_a + (lf_i64)offs_b[row] + (j - la);
}

// bit i of two bitmaps laid end to end: a's na bits (all ones when a is absent), then b's
LISTFN bool ls_concat_bit(const lf_u8* a, lf_i64 na, const lf_u8* b, lf_i64 i) { return i < na ? ls_bit(a, i) : ls_bit(b, i - na); }
