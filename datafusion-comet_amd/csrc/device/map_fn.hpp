// The entry search of a map column: what m[k] / element_at(m, k) — sent as map_extract(m, k) — is computed with in the fused kernels (codegen.cpp scalar_func
// "map_extract"; included by the generated sources that call it as comet_map_fn.hpp).  A map is laid out as Arrow lays it out: int32 offsets, then the entries
// Struct(key, value); the chain's table carries the key and the value column of a map with flat keys and values as columns of their own (exec.cpp
// extend_struct_fields: virt_kid 0 and 1 of a Map), so row i's entries are key / value rows off[i] … off[i + 1].
//   mf_find        the entry row of the FIRST entry, in entry order, whose key equals k: -1 when the map is NULL, when there is none, and for an empty map.
//                  The map's validity is read before its offsets and before any entry: a NULL map's offsets may span garbage.  Keys are never NULL (Arrow's
//                  map layout and Spark both forbid it), so no key validity is read.  A duplicate key — a Parquet file or an Arrow input may hold one — answers
//                  with its first entry.
//   utf8_eq_rows   value i of Utf8 column A equals value j of Utf8 column B: the lengths first, then the bytes
// One lane per row walks its own entries.  Neighbouring lanes read neighbouring entry rows (lane l's entries follow lane l - 1's), so a wave's loads of a short
// map fall into the same few cache lines although every lane's address is its own; the loop's trip count differs per lane, and a wave runs as long as its
// longest map — a row with thousands of entries is walked by one lane while 63 wait (DESIGN §6c has the measured figure).  No LDS, no cross-lane operation:
// EXEC is partial inside the loop.
// Plain C++ over CometCol (kparams.h): CDEV is comet_device.hpp's `__device__ __forceinline__` in a generated kernel and `inline` on the host, where
// tests/host/map_fn_check.cpp runs the same text under the sanitizers.
#pragma once
#include "kparams.h"
#ifndef CDEV
#define CDEV inline
#endif
#ifndef COMET_GLOBAL
#define COMET_GLOBAL
#endif
typedef unsigned char mf_u8;
typedef int mf_i32;
typedef long long mf_i64;
typedef unsigned long long mf_u64;
typedef __int128 mf_i128;

// how a key column is read, one per key representation; T is what the fused kernel computes the wanted key in (8- and 16-bit integers widen to i32)
struct MfBool {
  typedef bool T;
  static CDEV T at(const CometCol& c, mf_i64 e) {
    const mf_i64 j = c.offset + e;
    return (((const COMET_GLOBAL mf_u8*)c.data)[j >> 3] >> (j & 7)) & 1;
  }
};
struct MfI8 {
  typedef mf_i32 T;
  static CDEV T at(const CometCol& c, mf_i64 e) { return (mf_i32)((const COMET_GLOBAL signed char*)c.data)[c.offset + e]; }
};
struct MfI16 {
  typedef mf_i32 T;
  static CDEV T at(const CometCol& c, mf_i64 e) { return (mf_i32)((const COMET_GLOBAL short*)c.data)[c.offset + e]; }
};
struct MfI32 {      // Int32, Date
  typedef mf_i32 T;
  static CDEV T at(const CometCol& c, mf_i64 e) { return ((const COMET_GLOBAL mf_i32*)c.data)[c.offset + e]; }
};
struct MfI64 {      // Int64, Timestamp, TimestampNTZ
  typedef mf_i64 T;
  static CDEV T at(const CometCol& c, mf_i64 e) { return ((const COMET_GLOBAL mf_i64*)c.data)[c.offset + e]; }
};
struct MfDec64 {      // Decimal128 of up to 18 digits: the upper limb is sign extension
  typedef mf_i64 T;
  static CDEV T at(const CometCol& c, mf_i64 e) { return ((const COMET_GLOBAL mf_i64*)c.data)[2 * (c.offset + e)]; }
};
struct MfDec128 {      // Decimal128 beyond 18 digits: compared as 128-bit values
  typedef mf_i128 T;
  static CDEV T at(const CometCol& c, mf_i64 e) {
    const COMET_GLOBAL mf_u64* p = (const COMET_GLOBAL mf_u64*)c.data + 2 * (c.offset + e);
    return (mf_i128)(((unsigned __int128)p[1] << 64) | (unsigned __int128)p[0]);
  }
};

CDEV bool mf_valid(const CometCol& c, mf_i64 i) {
  const mf_i64 j = c.offset + i;
  return (((const COMET_GLOBAL mf_u8*)c.valid)[j >> 3] >> (j & 7)) & 1;
}

// row i's entries [first, end) of the map column m; false (and nothing but the validity bit read) for a NULL map.  `has_valid`: m.valid is a bitmap
CDEV bool mf_entries(const CometCol& m, bool has_valid, mf_i64 i, mf_i64& first, mf_i64& end) {
  first = end = 0;
  if (has_valid && !mf_valid(m, i)) return false;
  const COMET_GLOBAL mf_i32* off = (const COMET_GLOBAL mf_i32*)m.data + (m.offset + i);
  first = off[0];
  end = off[1];
  return true;
}

template <class R>
CDEV mf_i64 mf_find(const CometCol& m, bool has_valid, const CometCol& keys, mf_i64 i, typename R::T k) {
  mf_i64 e, end;
  if (!mf_entries(m, has_valid, i, e, end)) return -1;
  for (; e < end; e++)
    if (R::at(keys, e) == k) return e;
  return -1;
}

// value i of a Utf8 column against n literal bytes
CDEV bool mf_utf8_eq_lit(const CometCol& c, mf_i64 i, const char* lit, mf_i32 n) {
  const COMET_GLOBAL mf_i32* off = (const COMET_GLOBAL mf_i32*)c.data + (c.offset + i);
  const mf_i32 lo = off[0];
  if (off[1] - lo != n) return false;
  const COMET_GLOBAL mf_u8* p = (const COMET_GLOBAL mf_u8*)c.aux + lo;
  for (mf_i32 b = 0; b < n; b++)
    if (p[b] != (mf_u8)lit[b]) return false;
  return true;
}

CDEV bool utf8_eq_rows(const CometCol& a, mf_i64 i, const CometCol& b, mf_i64 j) {
  const COMET_GLOBAL mf_i32* oa = (const COMET_GLOBAL mf_i32*)a.data + (a.offset + i);
  const COMET_GLOBAL mf_i32* ob = (const COMET_GLOBAL mf_i32*)b.data + (b.offset + j);
  const mf_i32 alo = oa[0], n = oa[1] - alo, blo = ob[0];
  if (ob[1] - blo != n) return false;
  const COMET_GLOBAL mf_u8* p = (const COMET_GLOBAL mf_u8*)a.aux + alo;
  const COMET_GLOBAL mf_u8* q = (const COMET_GLOBAL mf_u8*)b.aux + blo;
  for (mf_i32 x = 0; x < n; x++)
    if (p[x] != q[x]) return false;
  return true;
}

// Utf8 keys: against a literal, and against row j of a Utf8 column
CDEV mf_i64 mf_find_lit(const CometCol& m, bool has_valid, const CometCol& keys, mf_i64 i, const char* lit, mf_i32 n) {
  mf_i64 e, end;
  if (!mf_entries(m, has_valid, i, e, end)) return -1;
  for (; e < end; e++)
    if (mf_utf8_eq_lit(keys, e, lit, n)) return e;
  return -1;
}
CDEV mf_i64 mf_find_row(const CometCol& m, bool has_valid, const CometCol& keys, mf_i64 i, const CometCol& kc, mf_i64 j) {
  mf_i64 e, end;
  if (!mf_entries(m, has_valid, i, e, end)) return -1;
  for (; e < end; e++)
    if (utf8_eq_rows(keys, e, kc, j)) return e;
  return -1;
}
