"""One small join per path of the hash join's host driver (csrc/exec_join.cpp): which table is built — LDS, chained, bucket (scrambling or monotone hash), direct map,
bitmap only, bucket table with key bitmap — and the steps around it (run counting, the probe sample, the output-capacity retry, the build-side tail with output growth,
the bucket-overflow fallback, the string dictionary).  Every case is checked against the oracle like tests/test_hash_join_gpu.py, and also asserts WHICH generated
kernels ran and how often (native.collect_kernel_times) and the join_* metrics: a restructuring of the driver that takes another path, or the same path with one
launch more, fails here even where the answer stays right.  The shapes are the smallest that select each path: 6 144 build rows is the LDS limit, 65 536 the bucket /
run-counting threshold, 2^20 probe rows with n >= 4 * B the sample gate.

Not covered: the CHAINED table with a key bitmap (k_jsample, k_jprobe_km) — by default it needs a build side whose runs exceed the bucket table's 16 384 partitions
(about 33 M runs), far above what a test may take; the process-wide COMET_JOIN_BUCKET_MIN_ROWS switch would reach it, but it is read once per process."""
import numpy as np
import pyarrow as pa
import pytest

from datafusion_comet_amd import native, serde as S
from tests.test_hash_join_gpu import CFIELDS, KFIELDS, _join_metrics, _oracle, _sorted, _sparse_dup_sides

pytestmark = pytest.mark.gpu

I32, I64 = S.T_INT32, S.T_INT64
K0 = [S.col(0, I64)]
COUNT = {"k_jbcnt": 1}
BUCKET = {"k_jphist": 1, "k_jpscat": 1, "k_jtbuild": 1}
TAIL = {"k_jbcount": 1, "k_jbscan": 1, "k_jbemit": 1}


def _side(keys, seed, mask=None):
    """k, v, id (CFIELDS)"""
    rng = np.random.default_rng(seed)
    n = len(keys)
    return pa.table({"k": pa.array(np.asarray(keys, dtype=np.int64), mask=mask), "v": pa.array(rng.integers(-1000, 1000, n), pa.int32()), "id": pa.array(np.arange(n, dtype=np.int64))})


def _check(plan, tables, ncols, kernels, **metrics):
    """runs the plan; the answer is the oracle's, the join's generated kernels (k_j…) and their call counts are `kernels`, the named join_* metrics as given"""
    with native.collect_kernel_times() as kt:
        got, m = _join_metrics(plan, tables, ncols)
    want = _oracle(plan, tables)
    calls = {k: v["calls"] for k, v in kt.times.items() if k.startswith("k_j")}
    assert calls == kernels, calls
    for name, v in metrics.items():
        assert m["join_" + name] == v, (name, m)
    assert (got.num_rows if got is not None else 0) == want.num_rows
    if want.num_rows:
        assert _sorted(got).equals(_sorted(want))
    return got


def _join(jt=S.INNER, build=S.BUILD_RIGHT, fields=CFIELDS, keys=K0, cond=None):
    return S.hash_join(S.scan(fields), S.scan(fields), keys, keys, jt, build, cond)


def test_small_build_side_is_probed_in_lds(built):
    rng = np.random.default_rng(1)
    build_t, probe_t = _side(rng.integers(0, 800, 1000), 2, rng.random(1000) < 0.02), _side(rng.integers(-5, 1000, 5000), 3, rng.random(5000) < 0.02)
    got = _check(_join(), [probe_t, build_t], 6, {"k_jlds": 1}, direct_maps=0, bucket_tables=0, bitmap_only=0, build_rows=1000, probe_rows=5000)
    assert got.num_rows > 1000


def test_chained_table_below_the_counting_threshold(built):
    rng = np.random.default_rng(4)
    build_t, probe_t = _side(rng.integers(0, 9000, 10_000), 5, rng.random(10_000) < 0.02), _side(rng.integers(-5, 12_000, 20_000), 6, rng.random(20_000) < 0.02)
    got = _check(_join(), [probe_t, build_t], 6, {"k_jbuild": 1, "k_jprobe": 1}, direct_maps=0, bucket_tables=0, mono_tables=0, bitmap_only=0)
    assert got.num_rows > 10_000


def test_bucket_table_with_the_scrambling_hash(built):
    probe_t, build_t = _sparse_dup_sides(70_000, 20_000, 7)
    keys = [S.col(0, I64), S.col(1, I32)]      # two key columns: no key range, no monotone hash
    _check(_join(fields=KFIELDS, keys=keys), [probe_t, build_t], 8, {**COUNT, **BUCKET, "k_jprobe_b": 1}, bucket_tables=1, mono_tables=0, direct_maps=0)


def test_bucket_table_with_the_monotone_hash(built):
    rng = np.random.default_rng(8)
    nb = 70_000
    base = rng.integers(0, 1000 * nb, 50_000)                  # one Int64 key, duplicates, spread evenly over a range of more than 64 bits per build row (no bitmap)
    build_t = _side(base[rng.integers(0, len(base), nb)], 9, rng.random(nb) < 0.01)
    probe_t = _side(np.where(rng.random(20_000) < 0.5, base[rng.integers(0, len(base), 20_000)], rng.integers(0, 1000 * nb, 20_000)), 10)
    _check(_join(), [probe_t, build_t], 6, {**COUNT, **BUCKET, "k_jprobe_b": 1}, bucket_tables=1, mono_tables=1, direct_maps=0)


def test_monotone_hash_refused_then_the_scrambling_hash(built):
    rng = np.random.default_rng(11)
    nb = 70_000
    bk = rng.permutation(np.arange(nb, dtype=np.int64) * 2)
    bk[5] = 1 << 40                                             # all other keys would land in the first partition
    build_t, probe_t = _side(bk, 12), _side(np.concatenate([rng.integers(-10, 2 * nb + 10, 20_000), [1 << 40, (1 << 40) + 1]]), 13)
    _check(_join(), [probe_t, build_t], 6, {**COUNT, **BUCKET, "k_jphist": 2, "k_jprobe_b": 1}, bucket_tables=1, mono_tables=0, direct_maps=0)


def _unique_keys(rng, nb):
    return rng.permutation(np.arange(1000, 1000 + 3 * nb, 3, dtype=np.int64))      # unique, every third key of the range, shuffled


def test_unique_key_goes_through_the_direct_map(built):
    rng = np.random.default_rng(14)
    nb = 70_000
    build_t = _side(_unique_keys(rng, nb), 15, rng.random(nb) < 0.01)
    pk = rng.integers(0, 1000 + 3 * nb + 2000, 20_000)
    pk[:4] = [-5, 0, 999, 1000 + 3 * nb + 1999]
    probe_t = _side(pk, 16, rng.random(20_000) < 0.02)
    got = _check(_join(), [probe_t, build_t], 6, {**COUNT, "k_jbmap": 1, "k_jdrows": 1, "k_jdprobe": 1}, direct_maps=1, bucket_tables=0, bitmap_only=0)
    assert got.num_rows > 1000


def test_direct_map_attempt_with_one_key_twice_builds_the_bucket_table(built):
    rng = np.random.default_rng(17)
    nb = 70_000
    bk = _unique_keys(rng, nb)
    bk[nb // 2] = bk[7]                                         # far apart: no run, found by the bitmap's build pass
    build_t = _side(bk, 18)
    probe_t = _side(np.concatenate([rng.integers(0, 1000 + 3 * nb + 2000, 20_000), np.full(5, bk[7])]), 19)
    _check(_join(), [probe_t, build_t], 6, {**COUNT, "k_jbmap": 1, "k_jdrows": 1, **BUCKET, "k_jprobe_bkm": 1}, direct_maps=0, bucket_tables=1)


@pytest.mark.parametrize("jt", [S.LEFT_SEMI, S.LEFT_ANTI])
def test_semi_and_anti_join_over_the_bitmap_alone(built, jt):
    rng = np.random.default_rng(20)
    nb = 70_000
    build_t = _side(rng.integers(0, nb, nb) * 3 + 1000, 21, rng.random(nb) < 0.01)      # a foreign key's shape: duplicates, holes
    pk = rng.integers(0, 1000 + 3 * nb + 2000, 20_000)
    pk[:4] = [-5, 0, 999, 1000 + 3 * nb + 1999]
    probe_t = _side(pk, 22, rng.random(20_000) < 0.02)
    got = _check(_join(jt), [probe_t, build_t], 3, {**COUNT, "k_jbmap": 1, "k_jprobe_bm": 1}, bitmap_only=1, bucket_tables=0, direct_maps=0)
    assert got.num_rows > 1000


def _clustered_build(rng, nb):
    """one Int64 key in a foreign key's range; twenty keys come twice, in neighbouring rows (runs: more keyed rows than leaders, so no direct map)"""
    keys = rng.permutation(nb - 20) * 2 + 1000
    return np.concatenate([np.repeat(keys[:20], 2), keys[20:]])


@pytest.mark.parametrize("present", [False, True])
def test_probe_sample_decides_on_the_key_bitmap(built, present):
    """2^20 probe rows over a 70 000-row bucket table: 8 192 of them go through the finished table first.  Fewer than half with a partner: the bitmap is built and the
    probe asks it first; nearly all with a partner: no bitmap."""
    rng = np.random.default_rng(23)
    nb, n = 70_000, 1 << 20
    bk = _clustered_build(rng, nb)
    build_t = _side(bk, 24)
    probe_t = _side(bk[rng.integers(40, nb, n)] if present else rng.integers(0, 16 * nb, n), 25)
    if present:
        _check(_join(), [probe_t, build_t], 6, {**COUNT, **BUCKET, "k_jsample_b": 1, "k_jprobe_b": 1}, bucket_tables=1, direct_maps=0)
    else:
        _check(_join(), [probe_t, build_t], 6, {**COUNT, **BUCKET, "k_jsample_b": 1, "k_jbmap": 1, "k_jprobe_bkm": 1}, bucket_tables=1, direct_maps=0)


def test_outer_tail_grows_the_output(built):
    rng = np.random.default_rng(26)
    build_t, probe_t = _side(rng.permutation(10_000), 27), _side(rng.integers(0, 20_000, 100), 28)
    got = _check(_join(S.FULL_OUTER), [probe_t, build_t], 6, {"k_jbuild": 1, "k_jprobe": 1, **TAIL}, bucket_tables=0)
    assert got.num_rows > 1024 + 100      # the unmatched build rows exceed what the probe's output buffers held


def test_probe_runs_again_when_its_output_exceeds_the_capacity(built):
    rng = np.random.default_rng(29)
    build_t, probe_t = _side(rng.integers(0, 10, 2000), 30), _side(rng.integers(0, 10, 2000), 31)
    got = _check(_join(), [probe_t, build_t], 6, {"k_jlds": 2})
    assert got.num_rows > 2000 + 1024


@pytest.mark.parametrize("jt", [S.LEFT_SEMI, S.LEFT_ANTI])
def test_semi_and_anti_join_built_on_the_left_emit_build_rows(built, jt):
    rng = np.random.default_rng(32)
    build_t, probe_t = _side(rng.integers(0, 8000, 10_000), 33, rng.random(10_000) < 0.02), _side(rng.integers(0, 16_000, 5000), 34)
    got = _check(_join(jt, S.BUILD_LEFT), [build_t, probe_t], 3, {"k_jbuild": 1, "k_jprobe": 1, **TAIL}, bucket_tables=0)
    assert 0 < got.num_rows < 10_000 and set(got.column(2).to_pylist()) <= set(range(10_000))


def test_long_utf8_keys_join_through_the_string_dictionary(built):
    rng = np.random.default_rng(35)
    words = [f"customer-{i:08d}-" + "x" * int(rng.integers(3, 14)) for i in range(4000)]      # 20 .. 30 bytes
    bs = [words[i] for i in rng.integers(0, len(words), 5000)]
    ps = [words[i] if rng.random() < 0.7 else f"nobody-{i:020d}" for i in rng.integers(0, len(words), 8000)]
    build_t = pa.table({"s": pa.array(bs, pa.string()), "id": pa.array(np.arange(len(bs), dtype=np.int64))})
    probe_t = pa.table({"s": pa.array(ps, pa.string()), "id": pa.array(np.arange(len(ps), dtype=np.int64))})
    plan = S.hash_join(S.scan([S.T_STRING, I64]), S.scan([S.T_STRING, I64]), [S.col(0, S.T_STRING)], [S.col(0, S.T_STRING)], S.INNER, S.BUILD_RIGHT)
    got, _ = _join_metrics(plan, [probe_t, build_t], 4)
    want = _oracle(plan, [probe_t, build_t])
    assert got.num_rows == want.num_rows > 1000 and _sorted(got).equals(_sorted(want))


def test_bucket_overflow_runs_both_attempts(built):
    """the inputs of test_hash_join_gpu.test_bucket_table_partition_overflow_takes_the_chained_table (same seed, same tables): the bucket table's build and probe, then —
    the probe's result says a partition overflowed — the chained table's, not counted again (150 000 rows are below the chained table's counting threshold)"""
    rng = np.random.default_rng(74)
    nb = 150_000
    build_t = pa.table({"k": pa.array(rng.integers(0, 3, nb).astype(np.int64) * (1 << 40)), "k2": pa.array(np.zeros(nb, np.int32)),
                        "v": pa.array(rng.integers(-1000, 1000, nb), pa.int32()), "id": pa.array(np.arange(nb, dtype=np.int64))})
    probe_t = pa.table({"k": pa.array(np.array([0, 1 << 40, 5, 2 << 40, 1 << 40], dtype=np.int64)), "k2": pa.array(np.zeros(5, np.int32)),
                        "v": pa.array(np.arange(5, dtype=np.int32)), "id": pa.array(np.arange(5, dtype=np.int64))})
    keys = [S.col(0, I64), S.col(1, I32)]
    _check(_join(fields=KFIELDS, keys=keys), [probe_t, build_t], 8, {**COUNT, **BUCKET, "k_jprobe_b": 1, "k_jbuild": 1, "k_jprobe": 2}, bucket_tables=0, direct_maps=0)
