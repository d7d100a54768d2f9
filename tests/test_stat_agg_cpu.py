"""var_samp / var_pop, stddev_samp / stddev_pop, covar_samp / covar_pop and corr without a GPU: createPlan accepts them in every aggregate mode,
plans the right state columns, refuses what it cannot run by name; serde.py's bytes follow the reference's schema; and the device helpers the
generated kernels call (comet_device.hpp "Statistical aggregates") are compiled for the host and checked against exact rationals."""
import ctypes
import os
import random
import subprocess
import sys
from fractions import Fraction

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from datafusion_comet_amd import native, serde as S  # noqa: E402

F64, I32, I64 = S.T_DOUBLE, S.T_INT32, S.T_INT64
x, y = S.col(0, F64), S.col(1, F64)
FUNCS = {
    "var_samp": lambda nz: S.variance(x, S.SAMPLE, nz), "var_pop": lambda nz: S.variance(x, S.POPULATION, nz),
    "stddev_samp": lambda nz: S.stddev(x, S.SAMPLE, nz), "stddev_pop": lambda nz: S.stddev(x, S.POPULATION, nz),
    "covar_samp": lambda nz: S.covariance(x, y, S.SAMPLE, nz), "covar_pop": lambda nz: S.covariance(x, y, S.POPULATION, nz),
    "corr": lambda nz: S.corr(x, y, nz),
}
WIDTH = {"var_samp": 3, "var_pop": 3, "stddev_samp": 3, "stddev_pop": 3, "covar_samp": 4, "covar_pop": 4, "corr": 6}


def state_scan(width, grouped):
    return S.scan(([I32] if grouped else []) + [F64] * width)


@pytest.mark.parametrize("name", sorted(FUNCS))
@pytest.mark.parametrize("nz", [True, False])
def test_accepted_in_every_mode(name, nz):
    agg = FUNCS[name](nz)
    w = WIDTH[name]
    for grouped in (False, True):
        keys = [S.col(2, I32)] if grouped else []
        partial = S.hash_agg(S.scan([F64, F64, I32]), keys, [agg])
        ok, text = native.check_plan(partial.encode())
        assert ok, text
        assert f"{name}_f64 -> (count" in text
        skeys = [S.col(0, I32)] if grouped else []
        for mode, label in ((S.FINAL, "agg(final)"), (S.PARTIAL_MERGE, "agg(partial-merge)")):
            ok, text = native.check_plan(S.hash_agg(state_scan(w, grouped), skeys, [agg], mode).encode())
            assert ok and label in text and name in text, text
    # mixed expr_modes (the count(DISTINCT) rewrite): a Partial count next to the PartialMerge statistical aggregate, whose state columns follow
    # the group column from initial_input_buffer_offset on
    child = S.scan([I32] + [F64] * w + [I64])
    mixed = S.hash_agg(child, [S.col(0, I32)], [agg, S.count(S.col(w + 1, I64))], S.PARTIAL, expr_modes=[S.PARTIAL_MERGE, S.PARTIAL], initial_input_buffer_offset=1)
    ok, text = native.check_plan(mixed.encode())
    assert ok and "agg(partial-merge)" in text, text


@pytest.mark.parametrize("name", sorted(FUNCS))
def test_codegen_reports_state_and_result_columns(name):
    agg = FUNCS[name](True)
    d = native.plan_codegen(S.hash_agg(S.scan([F64, F64, I32]), [S.col(2, I32)], [agg]).encode(), [True, True, False])
    states = d["out"][1:]
    assert len(states) == WIDTH[name] and all(o["type"] == S.DOUBLE and not o["nullable"] for o in states)
    assert len(d["fix_sums"]) == {3: 2, 4: 3, 6: 5}[WIDTH[name]]
    f = native.plan_codegen(S.hash_agg(state_scan(WIDTH[name], False), [], [agg], S.FINAL).encode(), [False] * WIDTH[name])
    assert [(o["type"], o["nullable"]) for o in f["out"]] == [(S.DOUBLE, True)]
    assert "comet::fix_addends_limbs" in d["source"] and "comet::fix_mean" in d["source"]


def test_shared_sums():
    """avg(x), var_samp(x) and stddev_samp(x) over one x share Σx and the count: three exact sums in all (Σx, Σx², and nothing else)"""
    d = native.plan_codegen(S.hash_agg(S.scan([F64, F64, I32]), [], [S.avg(x, F64, F64), S.variance(x), S.stddev(x), S.sum_(x, F64)]).encode(), [True, True, False])
    assert len(d["fix_sums"]) == 2


def test_refusals_name_their_reason():
    scan = S.scan([F64, F64, I32, I64])
    # two corrs over disjoint pairs and a float sum: 5 + 5 + 1 exact sums
    z = S.col(3, I64)
    ok, text = native.check_plan(S.hash_agg(scan, [], [S.corr(x, y), S.corr(S.cast(z, F64), S.cast(S.col(2, I32), F64)), S.sum_(S.col(2, I32), F64)]).encode())
    assert not ok and "more than 8 distinct Float64 sums" in text, text
    bad = S.variance(x)
    bad.stats_type = 2
    ok, text = native.check_plan(S.hash_agg(scan, [], [bad]).encode())
    assert not ok and "Unknown StatisticsType 2" in text, text
    ok, text = native.check_plan(S.hash_agg(scan, [], [S.stddev(S.col(2, I32))]).encode())
    assert not ok and "stddev_samp over Int32" in text, text
    ok, text = native.check_plan(S.hash_agg(scan, [], [S.covariance(x, z, S.POPULATION)]).encode())
    assert not ok and "covar_pop over Int64" in text, text
    # Cast(... AS double) children are what Spark's analyzer sends: accepted
    ok, text = native.check_plan(S.hash_agg(scan, [], [S.corr(S.cast(z, F64), S.cast(S.col(2, I32), F64))]).encode())
    assert ok, text
    # over a window frame: refused by name
    win = S.window(S.sort(scan, [(S.col(2, I32), False)]), [S.col(2, I32)], [(S.col(3, I64), False)],
                   [("agg", S.variance(x), F64, ("rows", "unbounded", "current"))])
    ok, text = native.check_plan(win.encode())
    assert not ok and "var_samp over a window frame" in text, text


def test_serde_bytes_parse_under_the_reference_schema():
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    from tests.test_proto_wire_cpu import unknown_paths
    fds = descriptor_pb2.FileDescriptorSet()
    with open(os.path.join(ROOT, "tests", "golden", "comet_protos.desc"), "rb") as f:
        fds.ParseFromString(f.read())
    pool = descriptor_pool.DescriptorPool()
    for fd in fds.file:
        pool.Add(fd)
    Agg = message_factory.GetMessageClass(pool.FindMessageTypeByName("spark.spark_expression.AggExpr"))
    for name, mk in FUNCS.items():
        for nz in (True, False):
            a = mk(nz)
            a.filter = S.gt(y, S.lit(0.0, F64))
            m = Agg()
            m.ParseFromString(a.encode())
            assert unknown_paths(m) == [], name
            which = m.WhichOneof("expr_struct")
            body = getattr(m, which)
            assert which == {"var_samp": "variance", "var_pop": "variance", "stddev_samp": "stddev", "stddev_pop": "stddev", "covar_samp": "covariance",
                             "covar_pop": "covariance", "corr": "correlation"}[name]
            assert body.null_on_divide_by_zero == nz and body.datatype.type_id == S.DOUBLE
            if which != "correlation":
                assert body.stats_type == (1 if name.endswith("pop") else 0)
            assert m.HasField("filter")


# --------------------------------------------------------------------------- the device helpers on the host

_HDR = os.path.join(ROOT, "datafusion-comet_amd", "csrc", "device", "comet_device.hpp")


@pytest.fixture(scope="module")
def dev(tmp_path_factory):
    src = open(_HDR).read()
    add = src[src.index("CDEV void acc_add192(u64* a, const u64* b) {"):src.index("CDEV void acc_umax128(")]
    fix = src[src.index("constexpr int kFixW = 158;"):src.index("// SumDecimal overflow is prefix-order dependent in the reference")]
    l0 = src.index("// Σ_j sext(w[j]) · 2^(43·j) as a 192-bit two's-complement number")
    limbs = src[l0:src.index("\n}\n", l0) + 3]
    stat = src[src.index("CDEV void two_prod(double a, double b, double& hi, double& lo)"):src.index("// (end of the statistical aggregates' helpers)")]
    shim = """
#include <stdint.h>
#include <string.h>
#include <math.h>
typedef long long i64; typedef unsigned long long u64; typedef int i32; typedef unsigned int u32; typedef short i16; typedef unsigned short u16;
typedef signed char i8; typedef unsigned char u8; typedef __int128 i128; typedef unsigned __int128 u128;
#define CDEV static inline
constexpr int kLimbBits = 43;
static inline i64 __double_as_longlong(double d) { i64 x; memcpy(&x, &d, 8); return x; }
static inline double __longlong_as_double(i64 v) { double x; memcpy(&x, &v, 8); return x; }
static inline double fp_mul(double a, double b) { return a * b; }
static inline double __dsqrt_rn(double a) { return sqrt(a); }
""" + add + fix + limbs + stat + """
extern "C" {
void t_two_prod(double a, double b, double* out) { two_prod(a, b, out[0], out[1]); }
// the grouped path: k addends → four limbs → 192 bits; the ungrouped path: k feeds into a 192-bit accumulator
void t_limbs(const double* xs, int k, int s, u64* out3) { u64 l[4]; fix_addends_limbs(xs, k, s, l); limbs_to_i192(l, 4, out3); }
void t_feed(const double* xs, int k, int s, u64* out3) { out3[0] = out3[1] = out3[2] = 0; for (int i = 0; i < k; i++) acc_feed_fix192(out3, xs[i], s); }
void t_limb_words(const double* xs, int k, int s, u64* l) { fix_addends_limbs(xs, k, s, l); }
// mean and m2 of xs[0..n) through the exact sums Σx (scale s1) and Σx² (scale s2, addends hi and lo)
void t_moments(const double* xs, int n, int s1, int s2, double* out) {
  u64 a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
  for (int i = 0; i < n; i++) {
    double h, l;
    two_prod(xs[i], xs[i], h, l);
    acc_feed_fix192(a, xs[i], s1);
    acc_feed_fix192(b, h, s2);
    acc_feed_fix192(b, l, s2);
  }
  out[0] = fix_mean(a, s1, 0, (u64)n);
  out[1] = fix_m2(b, s2, 0, a, s1, 0, (u64)n);
}
}
"""
    d = tmp_path_factory.mktemp("statdev")
    c = d / "stat_dev.cpp"
    c.write_text(shim)
    so = d / "libstatdev.so"
    subprocess.check_call(["g++", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unused-function", "-o", str(so), str(c)])
    m = ctypes.CDLL(str(so))
    dp, u64p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)
    m.t_two_prod.argtypes = [ctypes.c_double, ctypes.c_double, dp]
    for f in (m.t_limbs, m.t_feed, m.t_limb_words):
        f.argtypes = [dp, ctypes.c_int, ctypes.c_int, u64p]
    m.t_moments.argtypes = [dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp]
    return m


def _i192(w):
    v = w[0] | (w[1] << 64) | (w[2] << 128)
    return v - (1 << 192) if v >> 191 else v


def _ulp_distance(a: float, b: float) -> int:
    import struct
    k = lambda v: (lambda i: i if i >= 0 else -(i & 0x7FFFFFFFFFFFFFFF))(struct.unpack("<q", struct.pack("<d", v))[0])
    return abs(k(a) - k(b))


def test_two_prod_is_exact(dev):
    rnd = random.Random(1)
    out = (ctypes.c_double * 2)()
    for _ in range(2000):
        a = rnd.uniform(-1, 1) * 2.0 ** rnd.randint(-300, 300)
        b = rnd.uniform(-1, 1) * 2.0 ** rnd.randint(-300, 300)
        dev.t_two_prod(a, b, out)
        assert Fraction(out[0]) + Fraction(out[1]) == Fraction(a) * Fraction(b), (a, b)
        assert out[0] == a * b


def test_multi_addend_feed_is_the_exact_integer_sum(dev):
    """k addends of one row, truncated to the window 2^s each: the four limbs the grouped path adds, and the ungrouped path's k feeds, both hold
    Σ trunc(x_i / 2^s) exactly; every limb stays below 2^43 in magnitude"""
    rnd = random.Random(2)
    out3, outf, limbs = (ctypes.c_uint64 * 3)(), (ctypes.c_uint64 * 3)(), (ctypes.c_uint64 * 4)()
    for _ in range(3000):
        k = rnd.randint(1, 5)
        s = rnd.randint(-200, 100)
        xs = [rnd.choice([-1, 1]) * rnd.random() * 2.0 ** rnd.randint(s - 60, s + 157) for _ in range(k)]
        arr = (ctypes.c_double * k)(*xs)
        want = sum(int(Fraction(v) / Fraction(2) ** s) for v in xs)      # int() truncates toward zero, like the feed
        dev.t_limbs(arr, k, s, out3)
        dev.t_feed(arr, k, s, outf)
        assert _i192(out3) == want and _i192(outf) == want, (xs, s)
        dev.t_limb_words(arr, k, s, limbs)
        signed = [v - (1 << 64) if v >> 63 else v for v in limbs]
        assert all(0 <= v < 2**43 for v in signed[:3]) and abs(signed[3]) < 2**43, signed


def _exact_moments(xs):
    fr = [Fraction(v) for v in xs]
    n = len(fr)
    s1 = sum(fr)
    return s1 / n, sum(v * v for v in fr) - s1 * s1 / n


@pytest.mark.parametrize("case", ["2^30 + j/2", "prices", "random", "wide"])
def test_finisher_within_one_ulp(dev, case):
    rnd = random.Random(3)
    if case == "2^30 + j/2":      # mean² / variance ≈ 2^60: double-double would be hundreds of ulp off
        xs = [2.0**30 + j / 2 for j in range(8)]
    elif case == "prices":
        xs = [1e9 + rnd.randint(0, 10_000) / 100.0 for _ in range(2000)]
    elif case == "random":
        xs = [rnd.gauss(5.0, 3.0) for _ in range(3000)]
    else:
        xs = [round(rnd.uniform(-1, 1) * 2.0 ** (30 + rnd.randint(-20, 20))) / 2.0**30 for _ in range(3000)]
    # windows that hold every addend exactly: the lowest set bit of x and of x² (hi and lo)
    low = max(Fraction(v).denominator.bit_length() - 1 for v in xs)
    s1, s2 = -low, -2 * low
    out = (ctypes.c_double * 2)()
    dev.t_moments((ctypes.c_double * len(xs))(*xs), len(xs), s1, s2, out)
    mean, m2 = _exact_moments(xs)
    assert _ulp_distance(out[0], float(mean)) <= 1, (case, out[0], float(mean))
    assert _ulp_distance(out[1], float(m2)) <= 1, (case, out[1], float(m2))
