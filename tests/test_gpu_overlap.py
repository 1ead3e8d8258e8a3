"""The overlap step (`overlap`) through the HIP path: dcrx_overlap_run against the contract written in Python
(ou.expected_overlap) — the five planes, group_of, the public rows with their cells and the statistics, exactly, and the
invariants on every case — on degenerate sizes, two-sample extremes, duplicates in a sample, key identity, every setting of the
hash knob, limits, weights that need both product halves, the public rows' order and random tables; the pairs primitive on
crafted cells across the block boundary and on constructed cells (every plane size, blocks of several tiles, the group-end
look-up behind empty groups, full groups across tile edges, weights at the limit, a stream of the caller's, many blocks onto
one entry); the host entry on constructed tables (block edges, larger random tables, three hash bits at scale, a cell summed
over a thousand rows); and the sub-command end to end."""
import gzip
import os
import random

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import pipeline
from tests import overlap_util as ou
from tests import test_overlap as cpu

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -2


def _check(samples, classes, strings, S, weights=None, min_samples=2, want=None):
    """The native result against the contract (and the invariants on both); returns the expected (result, stats).
    want: ou.expected_overlap of the same arguments, where the caller has asserted a premise on it already."""
    w = [1 + (7 * k) % 13 for k in range(len(strings))] if weights is None else weights
    off, text = ou.row_text(strings)
    got = nat.overlap(samples, classes, off, text, w, S, min_samples)
    want = ou.expected_overlap(samples, classes, strings, w, S, min_samples) if want is None else want
    ou.assert_same(got, want, w)
    return want


def _refused(code, samples, classes, strings, S, weights, min_samples=1, off=None):
    o, text = ou.row_text(strings)
    with pytest.raises(nat.DcrxError) as e:
        nat.overlap(samples, classes, o if off is None else off, text, weights, S, min_samples)
    assert e.value.code == code, e.value


# ---- 1. degenerate sizes ----

def test_degenerate_sizes():
    for S in (1, 3):
        assert _check([], [], [], S, min_samples=1)[1]["groups"] == 0
    assert _check([0], [5], ["CASSF"], 1, min_samples=1)[1]["public_rows"] == 1
    strings = ["CASS" + ou.AMINO[k % 20] + ou.AMINO[(k // 20) % 20] for k in range(600)]      # 400 keys, 200 of them twice
    _, st = _check([0] * 600, [0] * 600, strings, 1, min_samples=1)
    assert st["groups"] == 400 and st["in_all_samples"] == 400
    _, st = _check([0, 2, 2, 0], [0] * 4, ["CASSA", "CASSA", "CASSB", "CASSC"], 3)      # sample 1 has no row
    assert st["rows_per_sample"] == [2, 0, 2] and st["shared_groups"] == 1 and st["in_all_samples"] == 0


# ---- 2. two-sample extremes ----

def test_two_sample_extremes():
    a = ["CASSA" + ou.AMINO[k % 20] * (1 + k // 20) for k in range(300)]
    b = ["CAWWA" + ou.AMINO[k % 20] * (1 + k // 20) for k in range(280)]
    res, st = _check([0] * 300 + [1] * 280, [0] * 580, a + b, 2)                        # nothing in common
    assert st["shared_groups"] == 0 and int(res["shared"][0][1]) == 0 and st["public_rows"] == 0
    res, st = _check([0] * 300 + [1] * 300, [0] * 600, a + a, 2)                        # identical
    assert st["shared_groups"] == st["groups"] == 300 and int(res["shared"][0][1]) == 300
    assert [int(x) for x in res["shared_weight"].reshape(-1)][0] == int(res["min_weight"][0][0])
    res, st = _check([0] * 300 + [1] * 90, [0] * 390, a + a[100:190], 2)                # a subset
    assert int(res["shared"][0][1]) == int(res["shared"][1][1]) == 90 and st["private_groups"] == 210


# ---- 3. duplicates in a sample ----

def test_duplicates_in_a_sample():
    strings, samples, w = ["CASSF"] * 4, [0, 0, 0, 1], [5, 7, 11, 3]
    res, st = _check(samples, [0, 0, 0, 0], strings, 2, w)      # `none`: three rows of sample 0 add
    assert st["groups"] == 1 and res["cell_weight"].tolist() == [23, 3] and int(res["min_weight"][0][1]) == 3
    assert int(res["prod_lo"][0][0]) == 23 * 23
    res, st = _check(samples, [0, 1, 0, 1], strings, 2, w)      # `vj`: the classes split them
    assert st["groups"] == 2 and res["group_of"].tolist() == [0, 1, 0, 1]
    assert res["head"].tolist() == [1] and res["cell_weight"].tolist() == [7, 3]
    _check([1, 0, 1, 0, 1, 1], [0] * 6, ["CASSF", "CASSF", "CASSY", "CASSF", "CASSF", "CASSY"], 2, min_samples=1)


# ---- 4. key identity ----

def test_key_identity():
    long_a = bytes((65 + k % 23) for k in range(300))
    long_b = long_a[:299] + b"!"
    strings = [b"CASS", b"CASSL", b"", b"CASS", b"CASSL", b"", b"CASS", long_a, long_b, long_a, b"CA\x80\xff", b"CA\x80\xfe",
               b"CA\x80\xff", b"CA\x00S", b"CA\x00S", b"CA\x00T", b"cass", b"CASS"]
    samples = [0, 0, 0, 1, 1, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 1, 1]
    classes = [0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    res, st = _check(samples, classes, strings, 3, min_samples=1)
    # CASS (class 0) / CASSL / "" / CASS (class 1) / long_a / long_b / ..ff / ..fe / CA\0S / CA\0T / cass
    assert st["groups"] == 11
    assert res["group_of"].tolist() == [0, 1, 2, 0, 1, 2, 3, 4, 5, 4, 6, 7, 6, 8, 8, 9, 10, 0]


# ---- 5. the hash knob ----

def test_hash_bits_do_not_enter_the_result():
    rnd = random.Random(21)
    keys = [(k % 3, "CASS" + ou.AMINO[k % 20] + ou.AMINO[k // 20]) for k in range(40)]
    rows = [keys[k % 40] for k in range(300)]
    rnd.shuffle(rows)
    samples = [rnd.randrange(4) for _ in rows]
    results = []
    try:
        for bits in (0, 3, 64):      # 0 bits: one run, and as many rounds as keys
            nat.overlap_set_hash_bits(bits)
            results.append(_check(samples, [c for c, _ in rows], [s for _, s in rows], 4, min_samples=1))
    finally:
        nat.overlap_set_hash_bits(64)
    assert results[0][1]["groups"] == 40
    for other in results[1:]:
        ou.assert_same(other, results[0])


# ---- 6. the pairs primitive on crafted cells ----

def _pairs(groups, S, start=None, stream=None, times=1, want=None):
    """The primitive over crafted cells against ou.expected_planes, every entry: `times` calls in a row on `stream` (a
    nat.Stream; None: the null stream) with ONE synchronisation after the last, onto `start`.  want: expected_planes(groups, S)
    where the caller has it already."""
    off, smp, wt = ou.cells_of_groups(groups)
    planes = np.zeros((5, S, S), np.uint64) if start is None else np.array(start, dtype=np.uint64)
    bufs = [nat.DeviceBuffer.from_host(a) for a in (off, smp, wt, planes)]
    try:
        for _ in range(times):
            nat.overlap_pairs_device(len(groups), bufs[0], bufs[1], bufs[2], S, bufs[3], None if stream is None else stream.ptr)
        if stream is None:
            nat.synchronize()
        else:
            stream.synchronize()
        got = bufs[3].to_host(np.uint64, 5 * S * S).reshape(5, S, S)
    finally:
        for b in bufs:
            b.free()
    want = ou.expected_planes(groups, S) if want is None else want
    onto = [0] * (5 * S * S) if start is None else [int(x) for x in np.asarray(start).reshape(-1)]
    assert [int(x) for x in got.reshape(-1)] == [o + times * x for o, x in zip(onto, (x for p in want for r in p for x in r))]
    return got


@pytest.mark.parametrize("front", [250, 255, 256])
def test_pairs_group_across_the_block_boundary(front):
    groups = [{k % 12: 1 + k % 9} for k in range(front)] + [{a: 100 + 3 * a for a in range(12)}] + [{5: 2}, {0: 1, 11: 4}]
    got = _pairs(groups, 12)
    assert int(got[0][0][11]) == 2


def test_pairs_64_samples_share_every_group():
    groups = [{a: 1 + (a * 7 + g) % 50 for a in range(64)} for g in range(300)]      # 19 200 cells, 75 tiles
    got = _pairs(groups, 64)
    assert int(got[0].min()) == 300


def test_pairs_add_onto_what_is_there_and_skip_empty_groups():
    start = (np.arange(5 * 9 * 9, dtype=np.uint64) * 1000 + 17).reshape(5, 9, 9)
    groups = [{0: 3, 8: 5}, {}, {}, {4: 0xFFFFFFFF, 8: 0xFFFFFFFF}] + [{}] * 300 + [{k % 9: 2} for k in range(280)] + [{1: 1, 2: 2, 3: 3}]
    _pairs(groups, 9, start)
    _pairs([{}, {}], 3)      # no cell at all
    nat.check(nat.lib().dcrx_overlap_pairs_device(0, None, None, None, 3, None, None))      # no group: nothing is launched
    for S in (0, 65):
        with pytest.raises(nat.DcrxError) as e:
            nat.check(nat.lib().dcrx_overlap_pairs_device(1, None, None, None, S, None, None))
        assert e.value.code == E_INVALID


# ---- 6b. the pairs primitive on constructed cells (tests/overlap_util.py: the lists, and the premise each list is for —
# asserted on the list and the Python reference before the device call; tests/test_overlap.py walks the same lists on the
# host).  The kernel's tile is ou.PAIR_BLOCK = 256 cells and its grid ou.PAIR_GRID = 2048 blocks at most. ----

@pytest.mark.parametrize("S", ou.PLANE_SIZES)
def test_pairs_every_plane_size(S):
    """Both sides of 8 | 9, 16 | 17 and 32 | 33 and the ends 1, 63, 64: every SMAX, PART 0 and PART 1, with the last sample in
    the triangle's last row and the full plane's last row and column."""
    groups, _, want = ou.constructed(f"plane_size_{S}")
    ou.premise_plane_size(groups, S, want)
    _pairs(groups, S, want=want)


def test_pairs_blocks_that_take_several_tiles():
    """More than PAIR_GRID tiles: blocks 0, 1 and 2 take a second tile, stage its ends again and go on adding to their planes."""
    groups, S, want = ou.constructed("several_tiles")
    ou.premise_several_tiles(groups, S, want)
    _pairs(groups, S, want=want)


@pytest.mark.parametrize("name", ou.LOOKUP_NAMES)
def test_pairs_group_end_look_up(name):
    """A group's end in the last staged slot (254 empty groups), behind it (255, 256: the search over cell_off), the same in a
    third tile (g_first > 0), empty groups that lead and that trail, and a tile of 256 single-cell groups."""
    groups, S, want = ou.constructed("lookup_" + name)
    ou.premise_lookup(name, groups)
    _pairs(groups, S, want=want)


@pytest.mark.parametrize("front", ou.TILE_EDGE_FRONTS)
def test_pairs_full_group_across_a_tile_edge(front):
    groups, S, want = ou.constructed(f"tile_edge_{front}")
    ou.premise_tile_edge(front, groups)
    _pairs(groups, S, want=want)


def test_pairs_full_groups_across_many_tile_edges():
    groups, S, want = ou.constructed("tile_edge_long")
    ou.premise_tile_edge_long(groups)
    _pairs(groups, S, want=want)


def test_pairs_weights_at_the_limit_in_full_groups():
    groups, S, want = ou.constructed("limit_weights")
    ou.premise_limit_weights(groups, want)
    _pairs(groups, S, want=want)


def test_pairs_on_a_stream_of_the_callers_twice_in_a_row():
    """Two calls on a stream of the caller's with no synchronisation between them, onto planes that are not zero."""
    groups, S, want = ou.constructed("plane_size_17")
    ou.premise_plane_size(groups, S, want)
    start = (np.arange(5 * S * S, dtype=np.uint64) * 1000 + 17).reshape(5, S, S)
    _pairs(groups, S, start, stream=nat.Stream(), times=2, want=want)


def test_pairs_many_blocks_onto_one_entry():
    """S = 1: 782 blocks flush onto the same four entries."""
    groups, S, want = ou.constructed("one_entry")
    ou.premise_one_entry(groups, want)
    _pairs(groups, S, want=want)


# ---- 6c. the host entry on constructed tables ----

@pytest.mark.parametrize("bits", [64, 0])
@pytest.mark.parametrize("m", [255, 256, 257, 513])
def test_tables_on_a_block_edge(m, bits):
    table = ou.block_edge_table(m)
    samples, classes, strings, w = table
    want = ou.expected_overlap(samples, classes, strings, w, 3, 1)
    ou.premise_block_edge(m, table, want)
    assert want[1]["groups"] == len(set(zip(classes, strings))) > 80      # at 0 bits: one run, and as many rounds as keys
    try:
        nat.overlap_set_hash_bits(bits)
        _check(samples, classes, strings, 3, w, min_samples=1, want=want)
    finally:
        nat.overlap_set_hash_bits(64)


@pytest.mark.parametrize("S,rows,pool,mode", [(8, 25000, 60000, "vj"), (8, 25000, 60000, "none"), (20, 5000, 30000, "vj")])
def test_larger_random_tables(S, rows, pool, mode):
    """S = 8: SMAX 8 at its edge; S = 20: SMAX 32 through the host entry."""
    samples, v, j, s, w = ou.random_tables(S, rows, pool, 7)
    classes = ou.call_classes(v, j, mode)
    want = ou.expected_overlap(samples, classes, s, w, S)
    st = want[1]
    assert st["shared_groups"] > 100 and st["private_groups"] > 100 and st["in_all_samples"] > 0 and st["largest_n_samples"] == S
    assert st["rows_in"] == S * rows
    _check(samples, classes, s, S, w, want=want)


def test_three_hash_bits_at_scale():
    samples, classes, strings, w = ou.hash_bits_table()
    want = ou.expected_overlap(samples, classes, strings, w, 4, 1)
    assert len(strings) == 6000 and want[1]["groups"] > 1800      # eight runs of more than 200 keys each: hundreds of rounds
    try:
        nat.overlap_set_hash_bits(3)
        _check(samples, classes, strings, 4, w, min_samples=1, want=want)
    finally:
        nat.overlap_set_hash_bits(64)


def test_a_cell_summed_over_many_rows():
    """1 000 rows of one cell — four blocks of the cell sort — add up to exactly 2^32 - 1; one unit more is refused."""
    table = ou.long_cell_table()
    samples, classes, strings, w = table
    want = ou.expected_overlap(samples, classes, strings, w, 3, 1)
    ou.premise_long_cell(table, want)
    _check(samples, classes, strings, 3, w, min_samples=1, want=want)
    samples, classes, strings, over = ou.long_cell_table(extra=1)
    assert sum(over) == sum(w) + 1 and max(over) < ou.LIMIT
    with pytest.raises(ou.Unsupported):
        ou.expected_overlap(samples, classes, strings, over, 3, 1)
    _refused(E_UNSUPPORTED, samples, classes, strings, 3, over)


# ---- 7. limits ----

def test_limits():
    strings = ["CASS" + ou.AMINO[k % 5] for k in range(64 * 3)]
    res, st = _check([k % 64 for k in range(192)], [0] * 192, strings, 64)      # S = 64: five keys, each in many samples
    assert st["groups"] == 5 and st["largest_n_samples"] > 32
    _refused(E_INVALID, [0], [0], ["CASS"], 65, [1])
    _refused(E_INVALID, [0], [0], ["CASS"], 0, [1])
    _refused(E_INVALID, [0, 3], [0, 0], ["CASS", "CASS"], 3, [1, 1])                  # a sample id equal to S
    _refused(E_INVALID, [0, 1], [0, 0], ["CASS", "CASS"], 2, [1, 1], off=np.array([4, 0, 4], np.uint64))
    _refused(E_INVALID, [0, 1], [0, 0], ["CASS", "CASS"], 2, [1, 1], min_samples=0)


# ---- 8. weights ----

def test_weights_that_need_both_product_halves():
    top = (1 << 32) - 1
    strings = ["CASSA", "CASSB", "CASSC"] * 2 + ["CASSD"]
    res, _ = _check([0, 0, 0, 1, 1, 1, 1], [0] * 7, strings, 2, [top] * 6 + [9])
    assert int(res["prod_hi"][0][1]) > 0
    assert (int(res["prod_hi"][0][1]) << 32) + int(res["prod_lo"][0][1]) == 3 * top * top > 1 << 64
    _refused(E_UNSUPPORTED, [0, 1], [0, 0], ["CASS", "CASS"], 2, [1 << 32, 1])
    _refused(E_UNSUPPORTED, [0, 1, 0], [0, 0, 0], ["CASS", "CASS", "CASS"], 2, [1 << 31, 1, 1 << 31])      # the CELL reaches 2^32
    _check([0, 1, 0], [0, 1, 0], ["CASS", "CASS", "CASS"], 2, [1 << 31, 1, (1 << 31) - 1])                # ... and one below it


# ---- 9. the public rows' order ----

def test_public_row_order():
    # heads 0 .. 5: (n_samples, weight) = (2, 10) (3, 6) (2, 10) (3, 6) (3, 9) (1, 50)
    rows = [(0, "K0", 4), (0, "K1", 2), (0, "K2", 5), (0, "K3", 1), (0, "K4", 3), (0, "K5", 50),
            (1, "K0", 6), (1, "K1", 2), (1, "K2", 5), (1, "K3", 2), (1, "K4", 3),
            (2, "K1", 2), (2, "K3", 3), (2, "K4", 3)]
    samples, strings, w = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    res, _ = _check(samples, [0] * len(rows), strings, 3, w, min_samples=2)
    assert res["head"].tolist() == [4, 1, 3, 0, 2]      # ties in n_samples and weight fall to the head
    res, st = _check(samples, [0] * len(rows), strings, 3, w, min_samples=1)
    assert res["head"].tolist() == [4, 1, 3, 0, 2, 5] and st["public_rows"] == st["groups"]
    res, _ = _check(samples, [0] * len(rows), strings, 3, w, min_samples=3)
    assert res["head"].tolist() == [4, 1, 3] and res["cell_sample"].tolist() == [0, 1, 2] * 3


# ---- 10. random tables ----

@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("mode", ["vj", "v", "none"])
def test_random_tables(seed, mode):
    samples, v, j, s, w = ou.random_tables(5, 2000, 3000, seed)
    res, st = _check(samples, ou.call_classes(v, j, mode), s, 5, w)
    assert st["shared_groups"] > 100 and st["private_groups"] > 100 and st["in_all_samples"] > 0


# ---- 11. end to end ----

def test_the_sub_command_end_to_end(tmp_path, capsys):
    files = cpu.write_inputs(tmp_path, cpu.HAND, gz=("B",))
    out = str(tmp_path / "out") + os.sep
    os.makedirs(out)
    pipeline.main(["overlap", "-in", *files, "-op", out, "-pf", "e_"])
    assert gzip.open(out + "e_overlap_pairs.tsv.gz", "rb").read() == cpu.HAND_PAIRS
    assert gzip.open(out + "e_overlap_public.tsv.gz", "rb").read() == cpu.HAND_PUBLIC
    assert "5 clonotypes" in capsys.readouterr().out
    pipeline.main(["overlap", "-in", *files, "-op", out, "-pf", "n_", "-dz", "--overlap-key", "none", "--min-samples", "3"])
    assert open(out + "n_overlap_public.tsv", "rb").read().decode().splitlines()[1:] == ["TRBV1\tTRBJ1\tCASSA\t3\t61\t11\t20\t30"]
