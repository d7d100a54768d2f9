"""The grouped aggregate's fixed-length-key variant without a GPU.  The executor generates it once it has verified (or predicted) one uniform length per Utf8
group key and the keys' bytes and null bits fit one word; comet_plan_codegen hands its text out under COMET_CODEGEN_STR_FIXED_LEN (a generator switch:
tools/codegen_corpus.py does not record under it).  Here:
  - the variant's text is pinned (tests/golden/grouped_fixed_key_codegen.json), and the text of the same plans WITHOUT the switch is what it was;
  - P::pack_key / P::unpack_key round-trip, and pack_key is injective, for every key shape the GPU test runs;
  - amax_enc is monotone over every bit-length boundary and rounding carry (an encode-once-per-lane maximum would rest on it; that lever did not clear its
    A/B noise and is not in the tree, the property stays checked);
  - the variant's per-row code, compiled for the host the way tests/emu/codegen_emu.py compiles generated code (its driver patched to send every key
    through pack_key / unpack_key), gives the oracle's answer."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pyarrow as pa
import pytest

from datafusion_comet_amd import native, serde as S, tpch
from tests import grouped_fixed_key_cases as C
from tests.emu import codegen_emu as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "grouped_fixed_key_codegen.json")
SWITCH = "COMET_CODEGEN_STR_FIXED_LEN"

# name → (plan, has_valid, the switch's value)
SHAPES = {
    "q1": (tpch.q1_plan, [False] * 7, "4:1,5:1"),
    "q1_nullable": (tpch.q1_plan, [True] * 7, "4:1,5:1"),
    "char3_char4": (C.keyed_plan, [False] * 4, "0:3,1:4"),
    "char1_char1_nullable": (C.keyed_plan, [True, True, False, False], "0:1,1:1"),
    "char4_char4_does_not_pack": (C.keyed_plan, [False] * 4, "0:4,1:4"),
    "one_key_of_two_is_variable": (C.keyed_plan, [False] * 4, "0:3"),
    "ansi": (C.ansi_plan, [False] * 6, "0:1,1:1"),
    "sum38": (C.sum38_plan, [False] * 3, "0:1,1:1"),
}


def _variant(monkeypatch, name):
    plan, hv, fixed = SHAPES[name]
    monkeypatch.setenv(SWITCH, fixed)
    try:
        return native.plan_codegen(plan().encode(), hv)
    finally:
        monkeypatch.delenv(SWITCH)


def test_variant_text_is_pinned_and_the_classic_text_is_what_it_was(built, monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    classic = {name: native.plan_codegen(plan().encode(), hv)["source"] for name, (plan, hv, _) in SHAPES.items()}
    # the classic text of Q1, against the record tests/test_codegen_corpus_cpu.py compares too
    with open(os.path.join(ROOT, "tests", "golden", "first_last_bit_agg_codegen.json")) as f:
        old = json.load(f)
    for name in ("q1", "q1_nullable"):
        assert (hashlib.sha256(classic[name].encode()).hexdigest(), len(classic[name].encode())) == (old[name]["sha256"], old[name]["bytes"]), name
    got = {}
    for name in SHAPES:
        src = _variant(monkeypatch, name)["source"]
        packs = "pack_key" in src
        assert packs == ("does_not_pack" not in name and "variable" not in name), name
        # what belongs to the variant comes with the packed key, and only with it
        assert ("unpack_key" in src) == packs, name
        assert ("ld_str_fixed" in src) and src != classic[name], name
        for word in ("pack_key", "ld_str_fixed"):
            assert word not in classic[name], (name, word)
        got[name] = {"sha256": hashlib.sha256(src.encode()).hexdigest(), "bytes": len(src.encode())}
    with open(GOLDEN) as f:
        want = json.load(f)
    assert got == want


# ---- the host build: tests/emu's driver, taught the variant's tile signature, plus entry points for pack_key / unpack_key and the amax helpers ----

def _patched_driver():
    d = E.DRIVER

    def swap(old, new):
        nonlocal d
        assert d.count(old) == 1, old
        d = d.replace(old, new)

    # a row's key goes through pack_key → unpack_key on its way into the driver's table, as it does on its way out of the device's LDS table
    swap("  std::vector<u64> k(key, key + P::NK);\n", "  std::vector<u64> k(key, key + P::NK);\n"
         "  if constexpr (comet::has_pack<P>::value) { u64 back[P::NK]; P::unpack_key(P::pack_key(k.data()), back); k.assign(back, back + P::NK); }\n")
    return d + r"""
extern "C" __attribute__((visibility("default"))) int emu_nk() { return P::NK; }
extern "C" __attribute__((visibility("default"))) unsigned long long emu_pack(const u64* key, u64* back) {
  if constexpr (comet::has_pack<P>::value) { const u64 w = P::pack_key(key); P::unpack_key(w, back); return w; }
  else return ~0ull;
}
extern "C" __attribute__((visibility("default"))) unsigned long long emu_amax_enc(u64 lo, u64 hi) { return comet::amax_enc(((u128)hi << 64) | lo); }
extern "C" __attribute__((visibility("default"))) int emu_amax_dec_covers(u64 lo, u64 hi) { const u128 a = ((u128)hi << 64) | lo; return comet::amax_dec(comet::amax_enc(a)) >= a; }
"""


@pytest.fixture
def host(monkeypatch):
    """run a plan's fixed-length-key variant on the host: tests/emu's run_chain over the text comet_plan_codegen hands out under the switch, with the patched driver"""
    monkeypatch.setattr(E, "DRIVER", _patched_driver())

    def run(name, table):
        plan, hv, fixed = SHAPES[name]
        real = native.plan_codegen

        def codegen(plan_bytes, has_valid):
            monkeypatch.setenv(SWITCH, fixed)
            try:
                d = real(plan_bytes, has_valid)
            finally:
                monkeypatch.delenv(SWITCH)
            assert "pack_key" in d["source"]
            return d

        monkeypatch.setattr(native, "plan_codegen", codegen)
        try:
            return E.run_chain(plan(), table)
        finally:
            monkeypatch.setattr(native, "plan_codegen", real)

    run.lib = lambda name: E._compiled(_variant(monkeypatch, name)["source"])
    return run


def _oracle(plan, table):
    from oracle import oracle as O
    return O.run_plan_to_arrow(S, plan, table)


@pytest.mark.parametrize("name,lens,nullable", [("q1", (1, 1), True), ("char3_char4", (3, 4), False), ("char1_char1_nullable", (1, 1), True)])
def test_pack_key_round_trips_and_is_injective(built, host, name, lens, nullable):
    lib = host.lib(name)
    lib.emu_nk.restype = ctypes.c_int
    lib.emu_pack.restype = ctypes.c_ulonglong
    lib.emu_pack.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    nk = lib.emu_nk()
    assert nk == 5
    rng = np.random.default_rng(5)
    seen = {}
    for trial in range(4000):
        key = np.zeros(nk, np.uint64)
        for j, L in enumerate(lens):
            null = nullable and rng.random() < 0.25
            if null:      # what lower_group_keys leaves of a NULL key: its bit in word 0, both of its words 0 — whatever bytes lie under the NULL
                key[0] |= np.uint64(1 << j)
            else:
                b = rng.integers(0, 256, L, dtype=np.uint64) if trial % 3 else np.full(L, 255 if trial % 2 else 0, np.uint64)
                key[1 + 2 * j] = sum(int(x) << (8 * i) for i, x in enumerate(b))
                key[2 + 2 * j] = np.uint64(L << 56)
        back = np.zeros(nk, np.uint64)
        w = lib.emu_pack(key.ctypes.data, back.ctypes.data)
        assert w < (1 << 63) and back.tolist() == key.tolist(), (key, back)
        assert seen.setdefault(w, key.tolist()) == key.tolist()      # injective: one word, one key
    assert len(seen) > 100


def _amax_lib(host):
    lib = host.lib("q1")
    lib.emu_amax_enc.restype = ctypes.c_ulonglong
    lib.emu_amax_enc.argtypes = [ctypes.c_ulonglong, ctypes.c_ulonglong]
    lib.emu_amax_dec_covers.argtypes = [ctypes.c_ulonglong, ctypes.c_ulonglong]
    return lib


def _boundary_values():
    M = (1 << 128) - 1
    vals = {0, 1, 2, 3, M, M - 1}
    for L in range(1, 129):
        lo, hi = 1 << (L - 1), (1 << L) - 1      # the smallest and the largest value of bit length L
        vals |= {lo, lo + 1, hi - 1, hi, (lo + hi) // 2}
        if L > 56:      # the rounding carry: leading 56 bits all ones; with and without bits below them
            top = ((1 << 56) - 1) << (L - 56)
            vals |= {top - 1, top, top + 1, top + (1 << (L - 57)), ((1 << 56) - 2) << (L - 56), (((1 << 56) - 2) << (L - 56)) + 1}
    return sorted(v for v in vals if 0 <= v <= M)


def test_amax_enc_is_monotone(built, host):
    """across every bit-length boundary from 1 to 128 and across the rounding carry: what reducing it with an unsigned max relies on"""
    lib = _amax_lib(host)
    enc = lambda a: lib.emu_amax_enc(a & ((1 << 64) - 1), a >> 64)
    vals = _boundary_values()
    words = [enc(a) for a in vals]
    assert all(w0 <= w1 for w0, w1 in zip(words, words[1:])), [(hex(a), hex(w)) for a, w in zip(vals, words)][:4]
    assert all(lib.emu_amax_dec_covers(a & ((1 << 64) - 1), a >> 64) for a in vals)
    assert enc(0) == enc(1) != 0


@pytest.mark.parametrize("mask", ["all", "alternating", "last_dead", "none"])
def test_q1_variant_on_the_host_matches_the_oracle(built, host, mask):
    n = 2 * C.TILE + 17
    table = C.q1_table(n, C.masks(n)[mask])
    got = host("q1", table)
    assert C.rows(got) == C.rows(_oracle(tpch.q1_plan(), table))
    assert got.num_rows == (0 if mask == "none" else 4)


@pytest.mark.parametrize("name,lens,nullable,groups", [("char3_char4", (3, 4), False, 70), ("char1_char1_nullable", (1, 1), True, 5)])
def test_keyed_variant_on_the_host_matches_the_oracle(built, host, name, lens, nullable, groups):
    n = C.TILE + 257
    table = C.keyed_table(n, lens[0], lens[1], groups, C.masks(n)["alternating"], nullable=nullable)
    assert C.rows(host(name, table)) == C.rows(_oracle(C.keyed_plan(), table))


def test_ansi_raise_sites_stay_under_the_filter_on_the_host(built, host):
    """rows that would raise lie below a Filter that drops them: no divide by zero, no overflow; the same rows alive raise"""
    n = C.TILE + 300
    offenders = [0, 63, 64, 255, 256, 511, 512, n - 1]
    table = C.ansi_table(n, offenders, live=False)
    assert C.rows(host("ansi", table)) == C.rows(_oracle(C.ansi_plan(), table))
    with pytest.raises(native.CometQueryExecutionException, match="DIVIDE_BY_ZERO|ARITHMETIC_OVERFLOW"):
        host("ansi", C.ansi_table(n, offenders, live=True))


@pytest.mark.parametrize("case,signs", [(c, s) for c in sorted(C.magnitudes()) for s in ("positive", "mixed") if s == "positive" or c.startswith("bits")])
def test_sum_overflow_verdicts_on_the_host(built, host, case, signs):
    table = C.sum38_table(case, signs)
    got = C.rows(host("sum38", table))
    assert got == C.rows(_oracle(C.sum38_plan(), table))
    assert case != "overflows" or all(r[2] is None for r in got)
