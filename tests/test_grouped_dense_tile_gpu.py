"""GPU: k_gagg's fixed-length-key variant — the LDS table probed on ONE packed key word, the grid sized
by occupancy — against the CPU oracle, bit for bit: row counts around the wave, the block and the tile; filter masks from none to all rows (16 ± 1 live lanes
per wave row, full and nearly empty tiles in turn, the chunk's last row dead and alive); key shapes that pack and one that does not; NULL keys over bytes that
stay in place; group counts on both sides of the private-copy and LDS-table sizes; ANSI raise sites on rows the Filter drops; sum magnitudes across the bit
lengths where amax_enc changes form; a wrong length prediction with packed keys.  (The masks were laid out for a dense-tile load path with a threshold of 16
lanes; that path measured slower and is not in the tree — profiles/q1_kgagg_critical_path.md — the cases stay.)"""
import numpy as np
import pyarrow as pa
import pytest

from datafusion_comet_amd import native, serde as S, tpch
from tests import grouped_fixed_key_cases as C

pytestmark = pytest.mark.gpu

D12, D38 = C.D12, C.D38


def _oracle(plan, table):
    from oracle import oracle as O
    return O.run_plan_to_arrow(S, plan, table)


def _run(plan, table, ncols):
    out = native.execute_to_table([native.DeviceInput(native.DeviceTable.from_arrow(table, "cuda:0"))], ncols, plan.encode())
    return pa.Table.from_batches(out) if out else None


@pytest.mark.parametrize("n", C.ROW_COUNTS)
def test_q1_row_counts_and_filter_masks(built, n):
    """Q1's plan (two CHAR(1) keys: the packed probe) over every row count, every mask: all / no rows pass, threshold − 1 / threshold / threshold + 1 live lanes
    per wave row, dense and sparse tiles in turn, the last row dead / alive under the clamp at n − 1.  The first task of the plan checks the lengths first, the
    later ones launch on the prediction: both launches of the variant run."""
    plan = tpch.q1_plan()
    for name, mask in C.masks(n).items():
        table = C.q1_table(n, mask)
        got, want = C.rows(_run(plan, table, tpch.Q1_NUM_OUTPUT_COLS)), C.rows(_oracle(plan, table))
        assert got == want, (n, name)
        assert (len(got) == 0) == (not mask.any())


@pytest.mark.parametrize("l1,l2,nullable", [(1, 1, False), (3, 4, False), (4, 4, False), (1, 1, True), (3, 4, True)])
@pytest.mark.parametrize("groups", [3, 5, 70, 300])
def test_key_shapes_and_group_counts(built, l1, l2, nullable, groups):
    """two CHAR(1) keys; CHAR(3) + CHAR(4) = 7 bytes, the widest that packs; CHAR(4) + CHAR(4), which does not pack and takes the five-word probe; the same with
    NULL keys whose bytes stay in place.  3 and 5 groups sit on either side of the private copies (GC = 4 here … 8), 70 and 300 on either side of the LDS
    table, so rows also reach the global table with a key rebuilt from its word."""
    n = 3 * C.TILE + 17
    plan = C.keyed_plan()
    table = C.keyed_table(n, l1, l2, groups, C.masks(n)["alternating"], nullable=nullable)
    got, want = C.rows(_run(plan, table, C.KEYED_NUM_OUTPUT_COLS)), C.rows(_oracle(plan, table))
    assert got == want
    assert len(got) >= min(groups, 3)


def test_ansi_raise_sites_stay_under_the_filter_in_a_dense_tile(built):
    """Rows that would raise (divide by zero, decimal overflow) sit in otherwise full tiles — at the tile's first and last lanes, the wave boundaries, the
    chunk's last row — below a Filter that drops exactly them: the task succeeds with the oracle's answer.  The same rows alive raise, so the first half
    proves something."""
    n = 2 * C.TILE + 300
    offenders = [0, 63, 64, 255, 256, 511, 512, 700, C.TILE + 511, n - 1]
    plan = C.ansi_plan()
    table = C.ansi_table(n, offenders, live=False)
    assert C.rows(_run(plan, table, 2 + 2 + 2 + 1)) == C.rows(_oracle(plan, table))
    with pytest.raises(native.CometQueryExecutionException, match="DIVIDE_BY_ZERO|ARITHMETIC_OVERFLOW"):
        _run(plan, C.ansi_table(n, offenders, live=True), 2 + 2 + 2 + 1)


# (next to the bound only all-positive sums: with mixed signs the verdict depends on the row order, and the engine refuses to decide, as it did)
@pytest.mark.parametrize("case,signs", [(c, s) for c in sorted(C.magnitudes()) for s in ("positive", "mixed") if s == "positive" or c.startswith("bits")])
def test_sum_overflow_bound_across_amax_bit_lengths(built, case, signs):
    """sum(decimal(38,6)) keeps max|v| for its overflow proof in one monotone word.  Magnitudes on both sides of the bit lengths at which
    amax_enc changes form (56 / 57: the mantissa starts to round; 64 / 65: the second limb), all-positive and mixed-sign, and sums on both sides of the
    38-digit bound: totals and NULL verdicts are the oracle's."""
    table = C.sum38_table(case, signs)
    plan = C.sum38_plan()
    got, want = C.rows(_run(plan, table, 2 + 2 + 1)), C.rows(_oracle(plan, table))
    assert got == want
    if case == "overflows":
        assert all(r[2] is None for r in got)


def test_wrong_prediction_with_packed_keys_gives_the_checked_answer(built):
    """CHAR(3) + CHAR(4) keys pack into one word.  Task 1 verifies the lengths; task 2 launches on them over a table whose second key's lengths are 2, 6, 2, 6, …
    (same byte total, same end points: the guard passes, the check beside k_gagg does not): the pass is voided and the answer is the check-first path's."""
    n = 2 * C.TILE + 2
    plan = C.keyed_plan()
    uni = C.keyed_table(n, 3, 4, 70, np.ones(n, bool))
    k2 = uni.column("k2").chunk(0)
    offs = 8 * (np.arange(n + 1, dtype=np.int64) // 2) + 2 * (np.arange(n + 1) % 2)
    alt = uni.set_column(1, "k2", pa.Array.from_buffers(pa.utf8(), n, [None, pa.py_buffer(offs.astype(np.int32).tobytes()), k2.buffers()[2]]))
    assert set(np.diff(offs).tolist()) == {2, 6} and offs[-1] == 4 * n
    assert C.rows(_run(plan, uni, C.KEYED_NUM_OUTPUT_COLS)) == C.rows(_oracle(plan, uni))
    with native.collect_kernel_times() as kt:
        got = _run(plan, alt, C.KEYED_NUM_OUTPUT_COLS)
    assert C.rows(got) == C.rows(_oracle(plan, alt))
    assert kt.times.get("k_gagg", {}).get("calls", 0) == 2      # the voided pass and the checked one
