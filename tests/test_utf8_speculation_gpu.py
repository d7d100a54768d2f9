"""GPU: the Utf8 length check of a device batch — one coalesced launch for all columns, and the speculation on top of it: a task whose plan has
verified a column's length before launches k_gagg's fixed-length variant at once, guarded, with the check of every offset beside it; a check that
disagrees voids the pass and the chunk runs again through what the check allows.  Every answer is compared bit-exact with the CPU oracle.

Which path ran shows in the launch counts: k_gagg launches once on a hit and on the check-first path, twice when a pass was voided; the check is ONE
launch per task either way.  (k_gagg's own launches are counted by name: a single chunk of 32 768 … 4 M rows first tries the partitioned kernels,
which kernel_stats() counts as a launch of its own, today as before.)"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pytest

from datafusion_comet_amd import native, serde as S, tpch

pytestmark = pytest.mark.gpu

TILE = 512                                  # rows of one k_gagg tile
SIZES = [1, TILE - 1, TILE + 1, 8 * TILE + 1, 300_001]
EVEN_SIZES = [2, TILE, TILE + 2, 8 * TILE + 2, 300_000]
PARTITIONED_MIN_ROWS = 32768                # below it kernel_stats() counts k_gagg alone


def _sweep(plan):
    """COMET_COMPILE_SWEEP=1 (tests/conftest.py): compile the plan instead of running it — before anything here touches a device."""
    if os.environ.get("COMET_COMPILE_SWEEP") == "1":
        native.Native.createPlan([], plan.encode())


def _rows(tbl):
    if tbl is None:
        return []
    cols = [tbl.column(i).to_pylist() for i in range(tbl.num_columns)]
    return sorted(zip(*cols), key=lambda r: tuple("" if x is None else str(x) for x in r[:3]))


_oracle_cache = {}


def _oracle_rows(plan, table, key):
    """rows of the CPU oracle's answer, computed once per (kind of table, n) and shared by the tests"""
    if key not in _oracle_cache:
        from oracle import oracle as O
        _oracle_cache[key] = _rows(O.run_plan_to_arrow(S, plan, table))
    return _oracle_cache[key]


def _utf8(offsets, data, n):
    return pa.Array.from_buffers(pa.utf8(), n, [None, pa.py_buffer(np.asarray(offsets, np.int32).tobytes()), pa.py_buffer(np.asarray(data, np.uint8).tobytes())])


def uniform_table(n):
    return tpch.lineitem_q1(n, seed=n)


def alternating_table(n):
    """l_returnflag with lengths 0, 2, 0, 2, …: the byte total and both end points are those of one byte per value"""
    assert n % 2 == 0
    t = uniform_table(n)
    data = np.frombuffer(t.column("l_returnflag").chunk(0).buffers()[2], np.uint8)[:n]
    offs = 2 * (np.arange(n + 1, dtype=np.int64) // 2)
    return t.set_column(4, "l_returnflag", _utf8(offs, data, n))


def two_byte_table(n):
    """l_returnflag with every value two bytes long: uniform, but not at the length seen before — the end points say so"""
    t = uniform_table(n)
    data = np.repeat(np.frombuffer(t.column("l_returnflag").chunk(0).buffers()[2], np.uint8)[:n], 2)
    return t.set_column(4, "l_returnflag", _utf8(2 * np.arange(n + 1, dtype=np.int64), data, n))


def run_task(plan_bytes, dev, ncols, make_input=native.DeviceInput):
    """one task → (result table or None, launches of k_gagg, launches kernel_stats() counts, check launches)"""
    with native.collect_kernel_times() as kt:
        it = native.CometExecIterator([make_input(dev)], ncols, plan_bytes)
        out = []
        while True:
            b = native.Native.executePlan(it.handle, ncols)
            if b is None:
                break
            out.append(b)
        launches = it.kernel_stats()[1]
        aux = it.aux_kernel_stats()[1]
        it.close()
    return (pa.Table.from_batches(out) if out else None), kt.times.get("k_gagg", {}).get("calls", 0), launches, aux


def _q1_task(table, **kw):
    dev = native.DeviceTable.from_arrow(table, "cuda:0")
    return run_task(tpch.q1_plan().encode(), dev, tpch.Q1_NUM_OUTPUT_COLS, **kw)


@pytest.mark.parametrize("n", SIZES)
def test_hit_launches_k_gagg_once(built, n):
    """Two tasks over the same uniform table: the second launches on the first's verdict.  Both are right, k_gagg runs once in each, the check once."""
    plan = tpch.q1_plan()
    _sweep(plan)
    table = uniform_table(n)
    want = _oracle_rows(plan, table, ("uniform", n))
    for _ in range(2):
        got, gagg, launches, aux = _q1_task(table)
        assert _rows(got) == want
        assert (gagg, aux) == (1, 1)
        if n < PARTITIONED_MIN_ROWS:
            assert launches == 1


@pytest.mark.parametrize("n", EVEN_SIZES)
def test_miss_with_intact_end_points_voids_the_pass(built, n):
    """After a uniform task, key lengths 0,2,0,2,…: the guard passes (the end points are those of one byte per value), the check beside k_gagg finds the
    column not uniform, the pass is voided — table, group counter, the overflow-proof words of sum_charge — and the chunk runs again through the offsets
    variant.  A third, uniform task is right again and checks first: the prediction was forgotten."""
    plan = tpch.q1_plan()
    _sweep(plan)
    uni, alt = uniform_table(n), alternating_table(n)
    got, gagg, _, aux = _q1_task(uni)
    assert _rows(got) == _oracle_rows(plan, uni, ("uniform", n)) and (gagg, aux) == (1, 1)
    got, gagg, launches, aux = _q1_task(alt)
    assert _rows(got) == _oracle_rows(plan, alt, ("alternating", n))
    assert (gagg, aux) == (2, 1)
    if n < PARTITIONED_MIN_ROWS:
        assert launches == 2
    got, gagg, _, aux = _q1_task(uni)
    assert _rows(got) == _oracle_rows(plan, uni, ("uniform", n)) and (gagg, aux) == (1, 1)


@pytest.mark.parametrize("n", SIZES)
def test_miss_at_the_end_points_fires_the_guard(built, n):
    """After a uniform task, every value of a key column two bytes long: last − first is 2 n, not n, so every workgroup of the guarded k_gagg leaves
    before it addresses a byte; the pass is void and the chunk runs again."""
    plan = tpch.q1_plan()
    _sweep(plan)
    uni, two = uniform_table(n), two_byte_table(n)
    got, gagg, _, aux = _q1_task(uni)
    assert _rows(got) == _oracle_rows(plan, uni, ("uniform", n)) and (gagg, aux) == (1, 1)
    got, gagg, _, aux = _q1_task(two)
    assert _rows(got) == _oracle_rows(plan, two, ("two_byte", n))
    assert (gagg, aux) == (2, 1)


class SlicedInput(native.DeviceInput):
    """the table handed over with Arrow offset SKIP on every column (the buffers stay whole)"""
    SKIP = 3

    def _get_next(self, _self, out):
        import ctypes
        rc = super()._get_next(_self, out)
        dev = ctypes.cast(out, ctypes.POINTER(native.ArrowDeviceArrayC)).contents
        if dev.array.release:
            dev.array.length -= self.SKIP
            for i in range(dev.array.n_children):
                child = dev.array.children[i].contents
                child.offset = self.SKIP
                child.length -= self.SKIP
        return rc


def test_sliced_column_is_checked_first(built):
    """A column with a non-zero Arrow offset is never launched on a prediction, whatever the plan has seen: it is checked first (one launch, offsets
    from the slice's first row on) and the answer is the oracle's over the slice."""
    plan = tpch.q1_plan()
    _sweep(plan)
    n = 8 * TILE + 1
    uni = uniform_table(n)
    got, gagg, _, aux = _q1_task(uni)
    assert _rows(got) == _oracle_rows(plan, uni, ("uniform", n)) and (gagg, aux) == (1, 1)
    got, gagg, launches, aux = _q1_task(uni, make_input=SlicedInput)
    assert _rows(got) == _oracle_rows(plan, uni.take(pa.array(range(SlicedInput.SKIP, n))), ("uniform_sliced", n))
    assert (gagg, launches, aux) == (1, 1, 1)


def test_three_keys_one_launch_reports_per_column(built, tmp_path):
    """Three Utf8 group keys, only the middle one not uniform: ONE launch checks all three and reports per column — the kernel that then runs reads
    columns 0 and 2 at their fixed lengths and column 1 through its offsets."""
    n = 4096
    k0 = ["x" if i % 3 else "y" for i in range(n)]
    k1 = ["" if i % 2 == 0 else "ab" for i in range(n)]
    k2 = ["pq" if i % 5 else "rs" for i in range(n)]
    t = pa.table({"k0": pa.array(k0, pa.string()), "k1": pa.array(k1, pa.string()), "k2": pa.array(k2, pa.string()), "v": pa.array(range(n), pa.int64())})
    plan = S.hash_agg(S.scan([S.T_STRING, S.T_STRING, S.T_STRING, S.T_INT64]), [S.col(0, S.T_STRING), S.col(1, S.T_STRING), S.col(2, S.T_STRING)],
                      [S.count(S.col(3, S.T_INT64))], mode=S.PARTIAL)
    _sweep(plan)
    want = {}
    for key in zip(k0, k1, k2):
        want[key] = want.get(key, 0) + 1
    want = sorted((a, b, c, cnt) for (a, b, c), cnt in want.items())
    dev = native.DeviceTable.from_arrow(t, "cuda:0")
    before = os.environ.get("COMET_JIT_DUMP_DIR")
    os.environ["COMET_JIT_DUMP_DIR"] = str(tmp_path)
    try:
        got, gagg, launches, aux = run_task(plan.encode(), dev, 4)
    finally:
        if before is None:
            del os.environ["COMET_JIT_DUMP_DIR"]
        else:
            os.environ["COMET_JIT_DUMP_DIR"] = before
    assert _rows(got) == want
    assert (gagg, launches, aux) == (1, 1, 1)
    sources = [open(os.path.join(tmp_path, f)).read() for f in os.listdir(tmp_path) if f.endswith(".hip")]
    fixed = [s for s in sources if "ld_str_fixed<" in s]
    assert len(fixed) == 1, "the variant this task compiled"
    loads = set(re.findall(r"ld_str_fixed<(\d+)>\(prm\.in\[(\d+)\]", fixed[0]))
    assert loads == {("1", "0"), ("2", "2")}
    assert "ld_str16(prm.in[1]" in fixed[0]
    # the next task cannot predict column 1 and checks first again; same answer
    got, gagg, launches, aux = run_task(plan.encode(), dev, 4)
    assert _rows(got) == want and (gagg, launches, aux) == (1, 1, 1)


def test_check_kernel_grid_stride_coverage(built):
    """The one-column call of the check kernel over more offsets than one sweep of its grid covers: 2048 workgroups × 4 waves × 8 loads × 64 lanes × 4
    offsets = 2^24 offsets per sweep, so 2^25 + 1000 values give every workgroup a second iteration and the first ones a ragged third.  A wrong
    offset in the second sweep, in the ragged tail, and none."""
    if os.environ.get("COMET_COMPILE_SWEEP") == "1":
        pytest.skip("compile sweep: no plan here")
    import ctypes
    import torch
    lib = native.lib()
    lib.comet_launch_utf8_uniform.restype = ctypes.c_int
    lib.comet_launch_utf8_uniform.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    sweep = 2048 * 4 * 8 * 64 * 4
    n = 2 * sweep + 1000
    offs = torch.arange(n + 1, dtype=torch.int32, device="cuda")

    def flag_of(buf):
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert lib.comet_launch_utf8_uniform(buf.data_ptr(), n, 1, flag.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        return int(flag.item())

    assert flag_of(offs) == 0
    for pos in (sweep + sweep // 2 + 77, n - 500):
        offs[pos] += 1                      # one offset off: value pos − 1 one byte longer, value pos one shorter — the end points stay
        assert flag_of(offs) != 0, pos
        offs[pos] -= 1
    assert flag_of(offs) == 0


_CHILD = """
import json, sys
sys.path.insert(0, {tests!r})
sys.path.insert(0, {root!r})
import datafusion_comet_amd
import test_utf8_speculation_gpu as T
from datafusion_comet_amd import tpch
n = {n}
out = []
for table in (T.uniform_table(n), T.alternating_table(n)):
    got, gagg, launches, aux = T._q1_task(table)
    out.append({{"rows": [[str(x) for x in r] for r in T._rows(got)], "gagg": gagg, "launches": launches, "aux": aux}})
print("RESULT " + json.dumps(out))
"""


def test_serial_path_in_a_fresh_process(built):
    """COMET_UTF8_SPECULATE=0 restores check-first for every task: the alternating table after a uniform one gives the same rows with a single k_gagg
    launch.  (The switch is read once per process, hence the child.)"""
    plan = tpch.q1_plan()
    _sweep(plan)
    n = 8 * TILE + 2
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, COMET_UTF8_SPECULATE="0")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(tests=here, root=os.path.dirname(here), n=n)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    for part, table, key in ((res[0], uniform_table(n), "uniform"), (res[1], alternating_table(n), "alternating")):
        want = [[str(x) for x in row] for row in _oracle_rows(plan, table, (key, n))]
        assert part["rows"] == want
        assert (part["gagg"], part["launches"], part["aux"]) == (1, 1, 1)
