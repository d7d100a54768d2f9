"""Float SUM / AVG over window frames without a GPU: createPlan accepts them over every frame shape and still refuses its neighbours by name,
and the per-row device math (csrc/device/window_fsum.hpp on the exact Float64 sums of comet_device.hpp), compiled for the host, yields for every
frame the exact real sum of its rows rounded once — bit for bit math.fsum — from DIFFERENCES of prefix sums, where prefix sums of doubles
already lose the 1.0 of 1e16, 1.0, −1e16."""
import ctypes
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from datafusion_comet_amd import native, serde as S  # noqa: E402
from tests.emu import codegen_emu as E  # noqa: E402

F64, F32, I32, I64 = S.T_DOUBLE, S.T_FLOAT, S.T_INT32, S.T_INT64
INF, NAN = float("inf"), float("nan")
FIELDS = [F64, F32, I32, I64]


def _window(fn):
    g, k = S.col(2, I32), S.col(3, I64)
    order = [(k, False, False)]
    return S.window(S.sort(S.scan(FIELDS), [(g, False, False)] + order), [g], order, [fn])


RANGE_VALUE = ("range", ("value", S.lit(3, I64)), ("value", S.lit(5, I64)))


@pytest.mark.parametrize("frame", [("rows", "unbounded", "current"), ("rows", -2, 2), RANGE_VALUE], ids=["running", "sliding", "range-value"])
def test_float_sum_and_avg_over_frames_are_planned(frame):
    x, x32 = S.col(0, F64), S.col(1, F32)
    for agg in (S.sum_(x, F64), S.avg(x, F64, F64), S.sum_(x32, F64), S.avg(x32, F64, F64)):
        ok, text = native.check_plan(_window(("agg", agg, F64, frame)).encode())
        assert ok, text
        assert "window: 1 function(s)" in text


def test_neighbours_stay_refused_by_name():
    x = S.col(0, F64)
    running = ("rows", "unbounded", "current")
    ok, text = native.check_plan(_window(("agg", S.sum_(S.lit(1.5, F64), F64), F64, running)).encode())
    assert not ok and "Window: SUM / AVG / MIN / MAX of a literal is not supported" in text, text
    ok, text = native.check_plan(_window(("agg", S.variance(x), F64, running)).encode())
    assert not ok and "var_samp over a window frame" in text, text
    ok, text = native.check_plan(_window(("agg", S.bit_or_agg(S.col(3, I64), I64), I64, running)).encode())
    assert not ok and "Window: aggregate (tag 10)" in text, text
    # the result of a float sum is Float64 whatever the argument's width; an integer average is still not a frame aggregate
    ok, text = native.check_plan(_window(("agg", S.avg(S.col(2, I32), F64, F64), F64, running)).encode())
    assert not ok and "over Int32 is not supported yet" in text, text


# --------------------------------------------------------------------------- the device math on the host

@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    csrc = os.path.join(ROOT, "datafusion-comet_amd", "csrc")
    so = str(tmp_path_factory.mktemp("window_fsum_emu") / "libwindow_fsum_emu.so")
    r = subprocess.run(["g++"] + E._FLAGS + ["-shared", "-I", E.HERE, "-I", E._workdir(), "-I", csrc, os.path.join(E.HERE, "window_fsum_emu.cpp"), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[:3000]
    lib = ctypes.CDLL(so)
    lib.window_fsum_emu.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]

    def run(values, frames, fn=0):
        """values: floats or None; frames: (start, end) pairs → ([result or None per frame], scale)"""
        x = np.array([0.0 if v is None else v for v in values], np.float64)
        bits = np.packbits(np.array([v is not None for v in values], np.uint8), bitorder="little") if len(values) else np.zeros(1, np.uint8)
        fr = np.array(frames, np.int64).reshape(-1, 2)
        out, ok = np.zeros(len(fr), np.float64), np.zeros(len(fr), np.uint8)
        windows = ctypes.c_int(0)
        s = lib.window_fsum_emu(x.ctypes.data if len(x) else None, bits.ctypes.data, len(x), fr.ctypes.data, len(fr), fn, out.ctypes.data, ok.ctypes.data, ctypes.byref(windows))
        run.windows = windows.value
        return [float(o) if k else None for o, k in zip(out, ok)], s
    return run


def exact_sum(rows):
    """the frame's SUM as Spark defines it: NULL without a non-NULL row, the IEEE outcome of its inf / NaN rows, else the correctly rounded exact sum"""
    xs = [v for v in rows if v is not None]
    if not xs:
        return None
    if any(math.isnan(v) for v in xs) or (INF in xs and -INF in xs):
        return NAN
    return math.fsum(xs)


def bits(v):
    return None if v is None else ("nan" if math.isnan(v) else struct.pack("<d", v))


def check_frames(emu, values, frames):
    got, _ = emu(values, frames)
    want = [exact_sum(values[a:b]) for a, b in frames]
    assert [bits(v) for v in got] == [bits(v) for v in want], [(f, g, w) for f, g, w in zip(frames, got, want) if bits(g) != bits(w)][:5]
    avg, _ = emu(values, frames, fn=1)
    for (a, b), g, w in zip(frames, avg, want):
        cnt = sum(v is not None for v in values[a:b])
        assert bits(g) == bits(None if w is None else w / cnt), (a, b, g, w, cnt)


def sliding(n, width):
    return [(max(0, i - width + 1), i + 1) for i in range(n)]


def test_cancellation_a_double_prefix_sum_loses(emu):
    values = [1e16, 1.0, -1e16, 3.0, 1e16, 0.5, -1e16, 2.0 ** -40, 7.0, -1e16, 1e16, 0.25]
    check_frames(emu, values, sliding(len(values), 3) + [(0, len(values)), (1, 4), (3, 8)])
    # a prefix sum of doubles has already lost the 1.0 at row 2: 1e16 + 1.0 − 1e16 comes out as 0.0
    prefix = np.cumsum(np.array(values))
    assert prefix[2] == 0.0 and math.fsum(values[0:3]) == 1.0


def test_subnormals_next_to_normals(emu):
    rnd = np.random.default_rng(5)
    values = [float(v) for v in rnd.integers(1, 1 << 52, 40) * 5e-324] + [float(v) for v in rnd.standard_normal(40) * 2.0 ** -1000] + [5e-324, -5e-324, 2.0 ** -1022, -(2.0 ** -975)]
    values = [values[i] for i in rnd.permutation(len(values))]
    check_frames(emu, values, sliding(len(values), 5) + sliding(len(values), 17) + [(0, len(values))])


def test_inf_and_nan_leave_with_their_rows(emu):
    values = [1.5, 2.25, INF, 4.0, 0.1, 0.2, -INF, INF, 0.3, 0.7, NAN, 1e-3, 1e3, None, -INF, 5.0, 6.0]
    frames = sliding(len(values), 3) + sliding(len(values), 2) + [(0, len(values)), (3, 6), (8, 10), (11, 14), (15, 17)]
    check_frames(emu, values, frames)
    got, _ = emu(values, [(2, 3), (6, 8), (10, 11), (3, 6), (11, 13)])
    assert got[0] == INF and math.isnan(got[1]) and math.isnan(got[2])
    assert got[3] == math.fsum([4.0, 0.1, 0.2]) and got[4] == math.fsum([1e-3, 1e3])      # finite again right behind the special rows


def test_null_and_empty_frames(emu):
    values = [None, None, 1.0, None, -0.0, 0.0, None, None]
    frames = [(0, 2), (0, 0), (3, 3), (8, 8), (3, 4), (6, 8), (0, 3), (4, 6), (4, 5), (0, 8)]
    got, _ = emu(values, frames)
    assert got == [None, None, None, None, None, None, 1.0, 0.0, 0.0, 1.0]
    assert bits(got[8]) == bits(0.0)              # a frame of zeros: +0.0, what the grouped sum yields
    check_frames(emu, values, frames)
    assert emu([None] * 5, [(0, 5), (1, 2)]) == ([None, None], 0)
    assert emu([], [(0, 0)])[0] == [None]


def test_truncation_when_one_column_spans_more_than_the_accumulator(emu):
    """2^-300 … 2^300 in one column: more than kFixW − 10 = 148 binary orders, where the shared rule alone (s = top + 2 − 158) would truncate the bits below
    2^s — and a truncated bit can decide a tie of the final rounding, one ulp of the RESULT, far beyond rows · 2^s.  The column is cut into windows 158 bits
    apart instead: every frame within rows · 2^s of the exact sum (the bound of the truncation regime), and in fact bit-equal to it"""
    rnd = np.random.default_rng(9)
    n = 400
    values = [float(m) * 2.0 ** int(e) for m, e in zip(rnd.standard_normal(n), rnd.integers(-300, 300, n))]
    values[10:30] = [float(v) * 2.0 ** 290 for v in rnd.standard_normal(20)]
    # two values near 2^274 that sum to an exact tie between two doubles, and a small one that decides it
    values[200:207] = [-2.948041241637928e-23, -2.037766852480794e-50, -7.815372586081521e+81, -2.7411800798215807e-31, 1.0631057878764206e+18, 9.457967568805706e-71,
                       3.943629562086103e+82]
    frames = sliding(n, 7) + [(0, n), (10, 30), (12, 19), (200, 207)]
    got, s = emu(values, frames)
    top = max(math.frexp(v)[1] for v in values)
    assert s == top + 2 - 158 and top - min(math.frexp(v)[1] - 53 for v in values) > 148 and emu.windows >= 4
    for (a, b), g in zip(frames, got):
        assert abs(g - math.fsum(values[a:b])) <= (b - a) * 2.0 ** s, (a, b, g)
    check_frames(emu, values, frames)
    # the whole range of doubles, subnormals to the largest: fourteen windows
    extreme = [5e-324, 1.7e308, -1.7e308, 2.5e-310, 1e300, 3.0, -1e-300, 1e-200]
    check_frames(emu, extreme, sliding(len(extreme), 3) + [(0, len(extreme)), (0, 2), (1, 4)])
    assert emu.windows == 14
