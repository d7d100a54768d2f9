// bloom_filter_agg (native/spark-expr/src/bloom_filter/{bloom_filter_agg,spark_bloom_filter,spark_bit_array}.rs) on gfx950: the hand-written kernels of
// exec_bloom.cpp.  The accumulator is one filter in device/bloom.hpp's layout (header words set by the host, bit words zeroed per execution):
//   bloom_put_kernel     rows of one integer column → k bits each (NULL rows skipped)
//   bloom_merge_kernel   ORs the big-endian words of one serialized state into the accumulator
//   bloom_finish_kernel  counts the set bits (Final: none → NULL) and writes Spark's serialization: big-endian header and words
// Two ways to set bits.  A filter of at most kBloomLdsWords words (8 KiB = 2^16 bits) is built per block in LDS and flushed with one atomicOr per
// non-zero word: at 8 KiB a block a CU still holds its eight blocks inside its 160 KiB, and a flush costs at most 1 024 atomics per block against
// thousands of rows.  Anything larger — Spark's default runtime filter is 2^23 bits = 1 MiB — sets its bits in global memory: a plain load first, the
// device-scope atomicOr only where the bit is not yet seen (bits are never cleared, so a stale line costs a redundant atomic at worst).
#include <hip/hip_runtime.h>

#include "device/comet_device.hpp"

using namespace comet;

namespace {

constexpr int kBloomLdsWords = 1024;

int grid_for(i64 n, i64 cap) {
  i64 g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// row i of an Int8 / Int16 / Int32 / Int64 column, sign-extended to a long
__device__ __forceinline__ i64 bloom_load(const void* __restrict__ vals, int width, i64 i) {
  switch (width) {
    case 1: return (i64)((const i8*)vals)[i];
    case 2: return (i64)((const i16*)vals)[i];
    case 4: return (i64)((const i32*)vals)[i];
    default: return ((const i64*)vals)[i];
  }
}

template <bool LDS>
__global__ __launch_bounds__(256) void bloom_put_kernel(const void* __restrict__ vals, int width, const u8* __restrict__ valid_bits, i64 first, i64 n, u64* __restrict__ f) {
  __shared__ u64 lds[LDS ? kBloomLdsWords : 1];
  const u64 version = f[0];
  const u32 k = (u32)f[1], seed = (u32)f[2], nwords = (u32)f[3];
  u64* const words = f + kBloomHeaderWords;
  if (LDS) {
    for (u32 w = threadIdx.x; w < nwords; w += 256) lds[w] = 0;
    __syncthreads();
  }
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
    const i64 row = first + i;
    if (valid_bits && !((valid_bits[row >> 3] >> (row & 7)) & 1)) continue;
    BloomIdx g = bloom_idx_begin(version, seed, nwords * 64u, bloom_load(vals, width, row));
    for (u32 j = 0; j < k; j++) {
      const u32 idx = bloom_idx_next(g);
      if (LDS) {
        const u64 bit = 1ull << (idx & 63);
        if (!(lds[idx >> 6] & bit)) atomicOr((unsigned long long*)&lds[idx >> 6], bit);
      } else {
        bloom_set(words, idx);
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (u32 w = threadIdx.x; w < nwords; w += 256) {
      const u64 v = lds[w];
      if (v && (words[w] & v) != v) atomicOr((unsigned long long*)&words[w], v);
    }
  }
}

// src: the first byte of a state's bit array (any alignment), nwords big-endian words; one state per launch, so a word has one writer
__global__ __launch_bounds__(256) void bloom_merge_kernel(const u8* __restrict__ src, i64 nwords, u64* __restrict__ words) {
  for (i64 w = (i64)blockIdx.x * 256 + threadIdx.x; w < nwords; w += (i64)gridDim.x * 256) {
    const u8* p = src + w * 8;
    u64 v = 0;
    for (int b = 0; b < 8; b++) v = (v << 8) | p[b];
    if (v) words[w] |= v;
  }
}

__device__ __forceinline__ u32 bswap32(u32 x) { return __builtin_bswap32(x); }

// out: header_bytes (12 for V1, 16 for V2) + 8 · nwords bytes, 4-byte aligned; *popcnt += the number of set bits
__global__ __launch_bounds__(256) void bloom_finish_kernel(const u64* __restrict__ f, u8* __restrict__ out, u64* __restrict__ popcnt) {
  const u32 version = (u32)f[0], k = (u32)f[1], seed = (u32)f[2], nwords = (u32)f[3];
  const u32 hdr = version == 2 ? 4 : 3;      // in 32-bit words
  u32* const o = (u32*)out;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    o[0] = bswap32(version);
    o[1] = bswap32(k);
    if (version == 2) o[2] = bswap32(seed);
    o[hdr - 1] = bswap32(nwords);
  }
  u32 bits = 0;
  for (i64 w = (i64)blockIdx.x * 256 + threadIdx.x; w < (i64)nwords; w += (i64)gridDim.x * 256) {
    const u64 v = f[kBloomHeaderWords + w];
    o[hdr + 2 * w] = bswap32((u32)(v >> 32));
    o[hdr + 2 * w + 1] = bswap32((u32)v);
    bits += (u32)__popcll(v);
  }
  __shared__ u32 part[256];
  part[threadIdx.x] = bits;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0 && part[0]) atomicAdd((unsigned long long*)popcnt, (unsigned long long)part[0]);
}

}  // namespace

extern "C" {

// width: bytes of one value (1, 2, 4, 8); first: the column's Arrow offset; f: the accumulator (header + words)
int comet_launch_bloom_put(const void* vals, int width, const uint8_t* valid_bits, int64_t first, int64_t n, uint64_t* f, int64_t nwords, void* stream) {
  if (n <= 0) return 0;
  if (nwords <= kBloomLdsWords) hipLaunchKernelGGL(bloom_put_kernel<true>, grid_for(n, 256 * 4), 256, 0, (hipStream_t)stream, vals, width, valid_bits, (i64)first, (i64)n, (u64*)f);
  else hipLaunchKernelGGL(bloom_put_kernel<false>, grid_for(n, 256 * 16), 256, 0, (hipStream_t)stream, vals, width, valid_bits, (i64)first, (i64)n, (u64*)f);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
int comet_launch_bloom_merge(const uint8_t* src_words, int64_t nwords, uint64_t* f, void* stream) {
  if (nwords <= 0) return 0;
  hipLaunchKernelGGL(bloom_merge_kernel, grid_for(nwords, 256 * 8), 256, 0, (hipStream_t)stream, src_words, (i64)nwords, (u64*)f + kBloomHeaderWords);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
int comet_launch_bloom_finish(const uint64_t* f, int64_t nwords, uint8_t* out, uint64_t* popcnt, void* stream) {
  hipLaunchKernelGGL(bloom_finish_kernel, grid_for(nwords, 256 * 8), 256, 0, (hipStream_t)stream, (const u64*)f, out, (u64*)popcnt);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
int comet_bloom_lds_words() { return kBloomLdsWords; }

}  // extern "C"
