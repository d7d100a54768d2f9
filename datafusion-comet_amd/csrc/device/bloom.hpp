// Spark's BloomFilter (BloomFilterImpl / BloomFilterImplV2; restated from native/spark-expr/src/bloom_filter/spark_bloom_filter.rs) over longs:
// the two scatter rules as an index generator, the bit test and the bit set, and the layout a filter has in device memory.  Shared by the fused
// kernels (might_contain lowers to bloom_might_contain over a bound buffer), by bloom_kernels.hip (bloom_filter_agg) and — compiled by g++ —
// by the host diagnostics of include/comet_amd.h.
//
// Device layout (native byte order, 8-byte aligned): kBloomHeaderWords u64 — version (1 | 2), k = numHashFunctions, seed (V2; 0 for V1), numWords —
// then numWords u64 of bits; bit i is words[i >> 6] & (1 << (i & 63)); bitSize = numWords · 64 < 2^31.  Everything a probe needs is read from that
// header: no generated kernel depends on a filter's size, k, version or contents.
//
// A long v hashes to h1 = murmur3_x86_32(8 LE bytes of v, seed), h2 = murmur3_x86_32(same bytes, h1) — mm3_hash_i64.
//   V1: for i = 1..k  c = (i32)h1 + i·(i32)h2 wrapping in 32 bits; c < 0 → ~c; index c % (i32)bitSize
//   V2: c = (i64)(i32)h1 · 0x7fffffff wrapping in 64 bits; k times: c += (i64)(i32)h2; ci = c < 0 ? ~c : c; index ci % (i64)bitSize
// Where bitSize is a power of two the remainder is a mask (the values are non-negative).
#pragma once

#ifndef CDEV      // the host build: the few names of comet_device.hpp this file uses
#define BLOOM_HOST 1
#define CDEV static inline
namespace comet {
typedef long long i64;
typedef unsigned long long u64;
typedef int i32;
typedef unsigned int u32;
CDEV u32 rotl32(u32 x, int r) { return (x << r) | (x >> (32 - r)); }
CDEV u32 mm3_mix_k1(u32 k1) { k1 *= 0xcc9e2d51u; k1 = rotl32(k1, 15); k1 *= 0x1b873593u; return k1; }
CDEV u32 mm3_mix_h1(u32 h1, u32 k1) { h1 ^= k1; h1 = rotl32(h1, 13); return h1 * 5u + 0xe6546b64u; }
CDEV u32 mm3_fmix(u32 h1, u32 len) {
  h1 ^= len; h1 ^= h1 >> 16; h1 *= 0x85ebca6bu; h1 ^= h1 >> 13; h1 *= 0xc2b2ae35u; h1 ^= h1 >> 16;
  return h1;
}
CDEV u32 mm3_hash_i64(i64 v, u32 seed) {
  u32 h = mm3_mix_h1(seed, mm3_mix_k1((u32)(u64)v));
  h = mm3_mix_h1(h, mm3_mix_k1((u32)((u64)v >> 32)));
  return mm3_fmix(h, 8u);
}
}  // namespace comet
#endif

namespace comet {

constexpr int kBloomHeaderWords = 4;      // version, k, seed, numWords
constexpr int kBloomMaxK = 255;           // bounds a row's loop (the planner and the binder refuse more)

// the k bit indices of one value, in Spark's order
struct BloomIdx {
  u32 h1, h2, bits, mask;   // mask: bits − 1 where bits is a power of two, else 0
  u32 i;                    // V1: the next multiplier
  i64 c;                    // V2: the running combined hash
  bool v2;
};
CDEV BloomIdx bloom_idx_begin(u64 version, u32 seed, u32 bits, i64 v) {
  BloomIdx g;
  g.h1 = mm3_hash_i64(v, seed);
  g.h2 = mm3_hash_i64(v, g.h1);
  g.bits = bits;
  g.mask = (bits & (bits - 1)) == 0 ? bits - 1 : 0;
  g.i = 1;
  g.v2 = version == 2;
  g.c = (i64)((u64)(i64)(i32)g.h1 * 0x7fffffffull);
  return g;
}
CDEV u32 bloom_idx_next(BloomIdx& g) {
  if (g.v2) {
    g.c = (i64)((u64)g.c + (u64)(i64)(i32)g.h2);
    const u64 ci = (u64)(g.c < 0 ? ~g.c : g.c);
    return g.mask ? (u32)ci & g.mask : (u32)(ci % g.bits);
  }
  i32 c = (i32)(g.h1 + g.i * g.h2);
  g.i++;
  if (c < 0) c = ~c;
  return g.mask ? (u32)c & g.mask : (u32)c % g.bits;
}

CDEV bool bloom_test(const u64* words, u32 idx) { return (words[idx >> 6] >> (idx & 63)) & 1; }
// bits are only ever set: a stale read costs a redundant atomic, never a lost bit
CDEV void bloom_set(u64* words, u32 idx) {
  const u64 bit = 1ull << (idx & 63);
#ifdef BLOOM_HOST
  words[idx >> 6] |= bit;
#else
  if (!(words[idx >> 6] & bit)) atomicOr((unsigned long long*)&words[idx >> 6], bit);
#endif
}

// f: a filter in the device layout.  True when every one of the k bits of v is set; leaves at the first clear one
CDEV bool bloom_might_contain(const u64* f, i64 v) {
  const u32 k = (u32)f[1];
  BloomIdx g = bloom_idx_begin(f[0], (u32)f[2], (u32)f[3] * 64u, v);
  const u64* words = f + kBloomHeaderWords;
  for (u32 j = 0; j < k; j++)
    if (!bloom_test(words, bloom_idx_next(g))) return false;
  return true;
}
// sets the k bits of v (f: header + words, as above)
CDEV void bloom_put(u64* f, i64 v) {
  const u32 k = (u32)f[1];
  BloomIdx g = bloom_idx_begin(f[0], (u32)f[2], (u32)f[3] * 64u, v);
  for (u32 j = 0; j < k; j++) bloom_set(f + kBloomHeaderWords, bloom_idx_next(g));
}

}  // namespace comet
