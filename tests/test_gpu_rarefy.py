"""`overlap --downsample` and `overlap --diversity` through the HIP path: dcrx_downsample and dcrx_downsample_device against
the contract written in Python (ru.expected_downsample: every key, sorted) — kept, reads, depth_used and threshold exactly, and
a sample's kept reads adding up to depth_used on every case — on degenerate tables, every depth of a small sample, the tile's
edges and the look-up behind the staged slots (the edges taken from the kernels' own constants), a skewed table, blocks that
take a second tile, 64 samples in one call, a selection that takes a second level, a stream of the caller's and a work space
one byte short; dcrx_abundance_classes against the contract; and the sub-command end to end."""
import os

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import pipeline
from tests import overlap_util as ou
from tests import rarefy_util as ru
from tests import test_rarefy as cpu

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -2


def _check(samples, weights, S, depths, seed, want=None):
    got = nat.downsample(samples, weights, S, depths, seed)
    want = ru.expected_downsample(samples, weights, S, depths, seed) if want is None else want
    ru.assert_same(got, want)
    ru.assert_sums(got, samples)
    return got


@pytest.mark.parametrize("name", ru.constructed_names())
def test_constructed_tables(name):
    """The degenerate tables and the tile's edges (tests/rarefy_util.py names what each is for)."""
    table, want = ru.constructed(name)
    ru.premise(name, table, want)
    _check(*table, want=want)


def test_every_depth_of_a_small_sample():
    """X = 37 in three rows, depths 0 .. 37: the threshold at the first and at the last rank, n = 1 and n = X - 1."""
    for n in range(38):
        got = _check([0, 0, 0], [10, 20, 7], 1, [n], 9)
        assert int(got["kept"].sum()) == n


def test_skewed_table():
    """One row holds 15 % of the reads beside 10^5 rows of 1 .. 40 reads; depths 10^3 and X / 2."""
    samples, weights = ru.skew_table()
    X = sum(weights)
    assert 0.149 < max(weights) / X < 0.151 and 2_000_000 < X < 4_000_000
    for depth in (1000, X // 2):
        got = _check(samples, weights, 1, [depth], 12)
        assert 0 < int(got["kept"][50000]) < weights[50000]


def test_blocks_take_a_second_tile():
    samples, weights = ru.second_tile_table()
    total, TILE, GRID = sum(weights), ru.constant("TILE"), ru.constant("GRID")
    assert -(-total // TILE) == GRID + 1 and total - 1 == GRID * TILE      # one read fewer and every block takes one tile
    _check(samples, weights, 1, [total // 3], 11)


def test_64_samples_of_unequal_size():
    samples, weights, depths = ru.many_samples_table()
    wants = {seed: ru.expected_downsample(samples, weights, 64, depths, seed) for seed in (21, 22)}
    reads, used = wants[21]["reads"], wants[21]["depth_used"]
    assert len({int(x) for x in reads}) == 64 and any(u == x for u, x in zip(used, reads)) and any(u == 0 for u in used)
    assert sum(0 < u < x for u, x in zip(used, reads)) >= 32      # half of the samples at least take part in the selection
    first = _check(samples, weights, 64, depths, 21, want=wants[21])
    other = _check(samples, weights, 64, depths, 22, want=wants[22])
    again = _check(samples, weights, 64, depths, 21, want=wants[21])
    real = [s for s in range(64) if 0 < used[s] < reads[s]]
    assert all(int(first["threshold"][s]) != int(other["threshold"][s]) for s in real)      # per sample: another seed, another threshold
    assert [int(x) for x in first["kept"]] == [int(x) for x in again["kept"]] != [int(x) for x in other["kept"]]


def _device_call(samples, weights, S, depths, seed, stream, bufs=None, short=0):
    m = len(samples)
    if bufs is None:
        work = nat.downsample_work_bytes(m, S)
        assert work > 0
        bufs = [nat.DeviceBuffer.from_host(np.asarray(a, dt)) for a, dt in ((samples, np.uint32), (weights, np.uint64), (depths, np.uint64))]
        bufs += [nat.DeviceBuffer(max(8 * n, 16)) for n in (m, S, S, S)] + [nat.DeviceBuffer(work), work]
    nat.downsample_device(S, m, *bufs[:3], seed, *bufs[3:7], bufs[7], bufs[8] - short, None if stream is None else stream.ptr)
    return bufs


def test_device_primitive_twice_in_a_row_on_a_stream_of_the_callers():
    """Two calls on one stream with no synchronisation between them, the second with another seed into the same arrays and the
    same work space: what comes back is the second call's."""
    samples, weights, depths = ru.many_samples_table()
    stream = nat.Stream()
    bufs = _device_call(samples, weights, 64, depths, 21, stream)
    _device_call(samples, weights, 64, depths, 22, stream, bufs)
    stream.synchronize()
    got = {k: b.to_host(np.uint64, n) for k, b, n in zip(ru.OUTPUTS, bufs[3:7], (len(samples), 64, 64, 64))}
    ru.assert_same(got, ru.expected_downsample(samples, weights, 64, depths, 22))
    ru.assert_sums(got, samples)


def test_a_work_space_one_byte_short_is_refused_not_launched():
    samples, weights, depths = [0, 0, 1], [5, 6, 7], [3, 3]
    bufs = _device_call(samples, weights, 2, depths, 1, None)
    nat.synchronize()
    before = bufs[3].to_host(np.uint64, 3)
    nat.check(nat.lib().dcrx_memset_device(bufs[3].ptr, 0xAB, 24))
    with pytest.raises(nat.DcrxError) as e:
        _device_call(samples, weights, 2, depths, 1, None, bufs, short=1)
    assert e.value.code == E_INVALID
    nat.synchronize()
    assert [int(x) for x in bufs[3].to_host(np.uint64, 3)] == [0xABABABABABABABAB] * 3 and int(before.sum()) == 6      # nothing ran


def test_a_selection_that_takes_a_second_level():
    """More keys in the threshold bin than are written out: the sample goes on to the next digit (the premise from the host
    walk; the totals of every other case stay below it)."""
    X = ru.constant("BINS") * ru.constant("CANDIDATES") * 21 // 20
    table = ([0, 0, 1], [X - 5, 5, 1000], 2, [X // 3, 10], 13)
    assert ru.host_downsample(*table, ru.constant("GRID"))[1] == [2, 1]
    _check(*table)


def test_host_entry_refusals():
    for args, code in ((([0, 1, 0], [1, 1, 1], 2, [1, 1], 1), E_INVALID), (([0, 1], [1 << 39, 1 << 39], 2, [1, 1], 1), E_UNSUPPORTED)):
        with pytest.raises(nat.DcrxError) as e:
            nat.downsample(*args)
        assert e.value.code == code


# ---- the abundance classes ----

def _classes(samples, groups, weights, S):
    got = nat.abundance_classes(samples, groups, weights, S)
    want = ru.expected_classes(samples, groups, weights, S)
    ru.assert_same_classes(got, want)
    return got


def test_classes_duplicates_zero_cells_and_the_limit():
    got = _classes([0, 0, 0, 1, 1, 2, 0], [5, 5, 9, 5, 7, 1, 9], [3, 4, 7, 0, 0, 2, 0], 4)      # (0, 5) and (0, 9) both add up to 7
    assert [int(x) for x in got["class_off"]] == [0, 1, 1, 2, 2] and [int(x) for x in got["class_mult"]] == [2, 1]
    top = (1 << 32) - 1
    got = _classes([1, 1, 1, 0], [4, 4, 4, 4], [top - 10, 4, 6, 1], 2)      # a cell that adds up to exactly 2^32 - 1
    assert [int(x) for x in got["class_count"]] == [1, top]
    with pytest.raises(nat.DcrxError) as e:                                  # ... and one unit more
        nat.abundance_classes([1, 1, 1, 0], [4, 4, 4, 4], [top - 10, 4, 7, 1], 2)
    assert e.value.code == E_UNSUPPORTED
    assert len(_classes([0, 1], [0, 0], [0, 0], 2)["class_count"]) == 0      # every cell dropped


@pytest.mark.parametrize("n", [255, 256, 257])
def test_classes_at_the_block_edge(n):
    rnd = np.random.default_rng(n)
    _classes(rnd.integers(0, 3, n), rnd.integers(0, 90, n), rnd.integers(0, 5, n), 3)


def test_classes_at_scale_equal_and_distinct_weights():
    rnd = np.random.default_rng(2)
    n = 200_000
    got = _classes(rnd.integers(0, 8, n), rnd.integers(0, 30_000, n), np.minimum(rnd.pareto(1.0, n).astype(np.uint64) + 1, 1 << 20), 8)
    assert len(got["class_count"]) > 500
    got = _classes(np.arange(3000) % 8, np.arange(3000), [6] * 3000, 8)      # all weights equal: one class per sample
    assert [int(x) for x in got["class_mult"]] == [375] * 8
    got = _classes(np.arange(3000) % 64, np.arange(3000), np.arange(1, 3001), 64)      # all weights distinct
    assert len(got["class_count"]) == 3000 and set(int(x) for x in got["class_mult"]) == {1}


# ---- the sub-command ----

def test_the_sub_command_end_to_end(tmp_path, capsys):
    tables = cpu.random_tables(seed=8, rows=(300, 120, 200))
    files = cpu.write_inputs(tmp_path, tables)
    out = str(tmp_path / "out") + os.sep
    os.makedirs(out)
    pipeline.main(["overlap", "-in", *files, "-op", out, "-pf", "e_", "-dz", "--downsample", "min", "--seed", "7", "--diversity"])
    reads = [sum(r[3] for r in rows) for _, rows in tables]
    kept, _ = cpu.kept_tables(tables, min(reads), 7)
    pairs, public = cpu.overlap_texts(kept)
    assert open(out + "e_overlap_pairs.tsv", "rb").read() == pairs and open(out + "e_overlap_public.tsv", "rb").read() == public
    samples = [s for s, (_, rows) in enumerate(kept) for _ in rows]
    rows = [r for _, t in kept for r in t]
    groups = ou.call_classes([r[0] + "|" + r[2] for r in rows], [r[1] for r in rows], "vj")
    ru.assert_diversity(open(out + "e_overlap_diversity.tsv", "rb").read(),
                        ru.diversity_rows("ABC", reads, ru.cells_of(samples, groups, [r[3] for r in rows], 3)))
    assert f"Downsampled to {min(reads):,} reads per sample (seed 7)" in capsys.readouterr().out
