"""A pure-Python model of Spark's BloomFilter over longs (BloomFilterImpl = V1, BloomFilterImplV2 = V2) and of bloom_filter_agg / might_contain as the
reference runs them (native/spark-expr/src/bloom_filter/*.rs, restated): the referee of tests/test_bloom_filter_{cpu,gpu}.py.

Serialized filter, all big-endian:  V1  i32 1 | i32 numHashFunctions | i32 numWords | numWords × i64
                                    V2  i32 2 | i32 numHashFunctions | i32 seed | i32 numWords | numWords × i64
Bit i is words[i >> 6] & (1 << (i & 63)); bitSize = numWords · 64."""
import math
import struct

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF


def _rotl32(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def _mix_k1(k1):
    k1 = (k1 * 0xCC9E2D51) & M32
    k1 = _rotl32(k1, 15)
    return (k1 * 0x1B873593) & M32


def _mix_h1(h1, k1):
    h1 ^= k1
    h1 = _rotl32(h1, 13)
    return (h1 * 5 + 0xE6546B64) & M32


def _fmix(h1, length):
    h1 ^= length
    h1 ^= h1 >> 16
    h1 = (h1 * 0x85EBCA6B) & M32
    h1 ^= h1 >> 13
    h1 = (h1 * 0xC2B2AE35) & M32
    h1 ^= h1 >> 16
    return h1


def murmur3_long(v: int, seed: int) -> int:
    """murmur3_x86_32 of the 8 little-endian bytes of the long v → u32"""
    u = v & M64
    h = _mix_h1(seed & M32, _mix_k1(u & M32))
    h = _mix_h1(h, _mix_k1(u >> 32))
    return _fmix(h, 8)


def _i32(u):
    u &= M32
    return u - (1 << 32) if u >> 31 else u


def _i64(u):
    u &= M64
    return u - (1 << 64) if u >> 63 else u


def indices(version: int, k: int, seed: int, bit_size: int, v: int):
    """the k bit indices of the long v, in Spark's order"""
    h1 = murmur3_long(v, seed if version == 2 else 0)
    h2 = murmur3_long(v, h1)
    out = []
    if version == 1:
        for i in range(1, k + 1):
            c = _i32(_i32(h1) + i * _i32(h2))
            if c < 0:
                c = ~c
            out.append(c % bit_size)
    else:
        c = _i64(_i32(h1) * 0x7FFFFFFF)
        for _ in range(k):
            c = _i64(c + _i32(h2))
            ci = ~c if c < 0 else c
            out.append(ci % bit_size)
    return out


def round_half_away(x: float) -> int:
    """f64::round: to the nearest integer, ties away from zero (|x| − floor|x| is exact, |x| + 0.5 is not)"""
    a = abs(x)
    r = int(math.floor(a)) + (1 if a - math.floor(a) >= 0.5 else 0)
    return r if x >= 0 else -r


def optimal_k(num_items: int, num_bits: int) -> int:
    return max(1, round_half_away(num_bits / num_items * math.log(2.0)))


class Filter:
    def __init__(self, version: int, k: int, num_words: int, seed: int = 0, words=None):
        self.version, self.k, self.seed = version, k, seed
        self.words = list(words) if words is not None else [0] * num_words

    @classmethod
    def for_agg(cls, num_items: int, num_bits: int, version: int = 0):
        """bloom_filter_agg's empty accumulator: the sizes truncated to i32, version 0 / 1 → V1, seed 0"""
        items, bits = _i32(num_items), _i32(num_bits)
        return cls(2 if version == 2 else 1, optimal_k(items, bits), (bits + 63) // 64)

    @classmethod
    def parse(cls, b: bytes):
        version, k = struct.unpack(">ii", b[:8])
        assert version in (1, 2), version
        off, seed = 8, 0
        if version == 2:
            seed, = struct.unpack(">i", b[8:12])
            off = 12
        n, = struct.unpack(">i", b[off:off + 4])
        words = struct.unpack(f">{n}Q", b[off + 4:off + 4 + 8 * n])
        return cls(version, k, n, seed, words)

    @property
    def bit_size(self):
        return len(self.words) * 64

    def put(self, v: int):
        for i in indices(self.version, self.k, self.seed, self.bit_size, v):
            self.words[i >> 6] |= 1 << (i & 63)

    def put_all(self, values):
        """NULL (None) inputs are ignored"""
        for v in values:
            if v is not None:
                self.put(v)
        return self

    def might_contain(self, v):
        if v is None:
            return None
        return all((self.words[i >> 6] >> (i & 63)) & 1 for i in indices(self.version, self.k, self.seed, self.bit_size, v))

    def merge(self, other: "Filter"):
        assert (self.version, self.k, self.seed, len(self.words)) == (other.version, other.k, other.seed, len(other.words))
        self.words = [a | b for a, b in zip(self.words, other.words)]
        return self

    def cardinality(self):
        return sum(bin(w).count("1") for w in self.words)

    def serialize(self) -> bytes:
        head = struct.pack(">ii", self.version, self.k) + (struct.pack(">i", self.seed) if self.version == 2 else b"")
        return head + struct.pack(">i", len(self.words)) + struct.pack(f">{len(self.words)}Q", *self.words)

    def final(self):
        """the Final aggregate's result: NULL when no bit is set"""
        return None if self.cardinality() == 0 else self.serialize()


# ---- the same rules over numpy arrays (the GPU tests' 100 000-row cases; tests/test_bloom_filter_cpu.py holds them to the scalar code above) ----

def _np():
    import numpy as np
    return np


def murmur3_long_np(v, seed):
    """v: int64 array, seed: u32 scalar or uint64 array of u32 values → uint64 array of u32 values"""
    np = _np()
    m32 = np.uint64(M32)

    def rotl(x, r):
        return ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & m32

    def mix_k1(k1):
        k1 = (k1 * np.uint64(0xCC9E2D51)) & m32
        return (rotl(k1, 15) * np.uint64(0x1B873593)) & m32

    def mix_h1(h1, k1):
        return (rotl(h1 ^ k1, 13) * np.uint64(5) + np.uint64(0xE6546B64)) & m32

    u = v.astype(np.int64).view(np.uint64)
    h = mix_h1(np.broadcast_to(np.asarray(seed, dtype=np.uint64) & m32, u.shape), mix_k1(u & m32))
    h = mix_h1(h, mix_k1(u >> np.uint64(32)))
    h = h ^ np.uint64(8)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m32
    h ^= h >> np.uint64(16)
    return h


def indices_np(version, k, seed, bit_size, v):
    """→ int64 array [len(v), k] of bit indices"""
    np = _np()
    with np.errstate(over="ignore"):
        h1 = murmur3_long_np(v, seed if version == 2 else 0)
        h2 = murmur3_long_np(v, h1)
        s1 = h1.astype(np.uint32).view(np.int32).astype(np.int64)
        s2 = h2.astype(np.uint32).view(np.int32).astype(np.int64)
        out = np.empty((len(v), k), dtype=np.int64)
        if version == 1:
            for i in range(1, k + 1):
                c = (s1 + i * s2).astype(np.int32).astype(np.int64)      # wraps to 32 bits
                c = np.where(c < 0, ~c, c)
                out[:, i - 1] = c % bit_size
        else:
            c = s1 * np.int64(0x7FFFFFFF)                                 # |s1| < 2^31: no 64-bit overflow yet
            for j in range(k):
                c = c + s2                                                # int64 addition wraps
                ci = np.where(c < 0, ~c, c)
                out[:, j] = ci % bit_size
        return out


def put_all_np(f: "Filter", values, valid=None):
    """values: int64 array; valid: boolean array or None"""
    np = _np()
    v = values if valid is None else values[valid]
    if len(v):
        idx = np.unique(indices_np(f.version, f.k, f.seed, f.bit_size, v).ravel())
        bits = np.zeros(f.bit_size, dtype=np.uint8)
        bits[idx] = 1
        words = np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view("<u8").ravel()
        f.words = [a | int(b) for a, b in zip(f.words, words)]
    return f


def might_contain_np(f: "Filter", values):
    """→ boolean array"""
    np = _np()
    words = np.array(f.words, dtype=np.uint64)
    idx = indices_np(f.version, f.k, f.seed, f.bit_size, values)
    hit = (words[idx >> 6] >> (idx & 63).astype(np.uint64)) & np.uint64(1)
    return hit.all(axis=1)
