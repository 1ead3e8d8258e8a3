"""`overlap --downsample` and `overlap --diversity` without a GPU: the key function on hand values, the shared code through
the host build (tests/host_rarefy), the primitive's steps walked on the host over the constructed tables, and the stage with
the native calls replaced by the Python contract (tests/rarefy_util.py)."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import overlap as ov
from decombinator_amd import pipeline
from tests import overlap_util as ou
from tests import rarefy_util as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELP_DIR = os.path.join(ROOT, "tests", "golden", "overlap_help")
M = ru.MASK

# computed once with Python integers from the two lines of the contract (include/dcrx.h "downsample")
FIN = [(0, 0), (1, 0x5692161D100B05E5), (M, 0xB4D055FCF2CBBD7B), (0x0123456789ABCDEF, 0xB2C058E4EBB5112C)]
KEYS = [((0, 0, 0), 0x1DF5DF97578D90C0),                      # seed 0
        ((M, 0, 0), 0x077CA23776407269),                      # seed 2^64 - 1: seed + step wraps
        ((1, 3, 5), 0xA2B8023F84E3C459),
        ((1, 0, (1 << 40) - 2), 0xBE36605D031B881F),          # the last read there can be: (r + 1) * step wraps many times
        ((7, 63, 1 << 63), 0x88F7AB977C88D217),               # (r + 1) * step wraps
        ((M, 4095, M - 1), 0x192252C9FDD85CE8)]               # r + 1 = 2^64 - 1


def test_key_function_on_hand_values():
    for z, want in FIN:
        assert ru.fin(z) == want
    for args, want in KEYS:
        assert ru.key(*args) == want
        assert int(ru.sample_keys(args[0], args[1], 6)[5]) == ru.key(args[0], args[1], 5)      # numpy's arithmetic is the same


def test_host_library_key_equals_python():
    H = ru.host_lib()
    for z, want in FIN:
        assert H.rarefy_host_fin(z) == want
    for args, want in KEYS:
        assert H.rarefy_host_key(*args) == want
    k = 0xFEDCBA9876543210
    bits = ru.constant("BINS").bit_length() - 1
    assert ru.constant("BINS") == 1 << bits
    for level in range(ru.constant("LEVELS")):
        assert H.rarefy_host_digit(k, level) == (k >> (64 - bits * (level + 1))) & (ru.constant("BINS") - 1)
        assert H.rarefy_host_prefix(k, level) == (k >> (64 - bits * level) if level else 0)
    assert 1 << (64 - bits * ru.constant("LEVELS")) <= ru.constant("CANDIDATES")      # the last level's bin can be written out


def test_keys_of_a_sample_are_distinct():
    """fin is a bijection and the multiplier of r + 1 is odd: no two reads of a sample share a key (no ties, no tie rule)."""
    for seed, s in ((0, 0), (1, 5), (M, 63)):
        assert len(np.unique(ru.sample_keys(seed, s, 1 << 20))) == 1 << 20
    assert ru.READ_STEP % 2 == 1 and ru.SAMPLE_STEP % 2 == 1
    # the inverse of fin's steps exists: an xor-shift is undone by repeating it, an odd multiplier by its inverse mod 2^64
    for mult in (0xBF58476D1CE4E5B9, 0x94D049BB133111EB):
        assert mult * pow(mult, -1, 1 << 64) % (1 << 64) == 1


def test_run_kept_exhaustively_on_small_masks():
    """A wave's runs: the kept reads between a head and the next head."""
    H = ru.host_lib()
    rnd = np.random.default_rng(5)
    for _ in range(200):
        heads = int(rnd.integers(0, 1 << 63)) | 1
        keeps = int(rnd.integers(0, 1 << 63)) << 1 | int(rnd.integers(0, 2))
        for lane in range(64):
            if not heads >> lane & 1:
                continue
            end = next((q for q in range(lane + 1, 64) if heads >> q & 1), 64)
            assert H.rarefy_host_run_kept(heads, keeps & M, lane) == sum(keeps >> q & 1 for q in range(lane, end))


def test_sanity_of_the_key():
    """Rows of 30 and 70 reads, depth 50, seeds 0 .. 999: the mean kept of row 0 is the hypergeometric 15 within [14.5, 15.5]
    (the standard deviation of that mean is 0.073; this key gives 15.222 on these seeds).  A condition, not a tuning."""
    total = 0
    for seed in range(1000):
        r = ru.expected_downsample([0, 0], [30, 70], 1, [50], seed)
        assert int(r["kept"].sum()) == 50
        total += int(r["kept"][0])
    assert 14.5 <= total / 1000 <= 15.5


@pytest.mark.parametrize("name", ru.constructed_names())
def test_host_walk_on_constructed_tables(name):
    table, want = ru.constructed(name)
    ru.premise(name, table, want)
    ru.assert_sums(want, table[0])
    for grid in (1, 3, ru.constant("GRID")):
        got, levels = ru.host_downsample(*table, grid)
        ru.assert_same(got, want)
        assert all(lv <= 1 for lv in levels)


def test_host_walk_every_depth():
    """X = 37 in three rows, every depth 0 .. 37: the threshold at the first and at the last rank."""
    keys = sorted(ru.key(9, 0, r) for r in range(37))
    for n in range(38):
        table = ([0, 0, 0], [10, 20, 7], 1, [n], 9)
        want = ru.expected_downsample(*table)
        assert int(want["threshold"][0]) == (keys[n] if n < 37 else M) and int(want["kept"].sum()) == n
        ru.assert_same(ru.host_downsample(*table, 3)[0], want)


def test_host_walk_second_tile_and_skew():
    samples, weights = ru.second_tile_table()
    total, tiles = sum(weights), -(-sum(weights) // ru.constant("TILE"))
    assert tiles == ru.constant("GRID") + 1 and -(-tiles // ru.constant("GRID")) == 2      # blocks take two tiles, from this total on
    table = (samples, weights, 1, [total // 3], 11)
    ru.assert_same(ru.host_downsample(*table, ru.constant("GRID"))[0], ru.expected_downsample(*table))
    samples, weights = ru.skew_table()
    assert 0.149 < max(weights) / sum(weights) < 0.151
    table = (samples, weights, 1, [1000], 12)
    ru.assert_same(ru.host_downsample(*table, ru.constant("GRID"))[0], ru.expected_downsample(*table))


def test_host_walk_takes_a_second_level():
    """A sample whose threshold bin holds more keys than are written out goes on to the next digit."""
    X = ru.constant("BINS") * ru.constant("CANDIDATES") * 21 // 20
    table = ([0, 0, 1], [X - 5, 5, 1000], 2, [X // 3, 10], 13)
    got, levels = ru.host_downsample(*table, ru.constant("GRID"))
    assert levels == [2, 1]
    ru.assert_same(got, ru.expected_downsample(*table))


# ---- the entries: refusals before the device ----

def test_abi_version_is_5():
    assert nat.ABI_VERSION == 5 and nat.lib().dcrx_abi_version() == 5
    assert nat.DOWNSAMPLE_MAX_SAMPLES == ru.constant("MAX_SAMPLES")


def test_entries_refuse_before_the_device():
    with pytest.raises(nat.DcrxError) as e:      # sample ids that go down
        nat.downsample([0, 1, 0], [1, 1, 1], 2, [1, 1], 1)
    assert e.value.code == -1
    with pytest.raises(nat.DcrxError) as e:      # a sample id equal to S
        nat.downsample([0, 2], [1, 1], 2, [1, 1], 1)
    assert e.value.code == -1
    for S in (0, nat.DOWNSAMPLE_MAX_SAMPLES + 1):
        with pytest.raises(nat.DcrxError) as e:
            nat.downsample([], [], S, [1] * S, 1)
        assert e.value.code == -1
    one = np.zeros(4, np.uint64)
    p = one.ctypes.data      # m >= 2^30 is refused by the argument alone: nothing behind the pointers is read
    assert nat.lib().dcrx_downsample(1, 1 << 30, p, p, p, 1, p, p, p, p) == -2
    assert nat.lib().dcrx_downsample_device(1, 1 << 30, p, p, p, 1, p, p, p, p, p, 1 << 40, None) == -2
    assert nat.lib().dcrx_downsample_device(0, 1, p, p, p, 1, p, p, p, p, p, 1 << 40, None) == -1
    assert nat.downsample_work_bytes(1 << 30, 1) == 0 and nat.downsample_work_bytes(1, 0) == 0
    with pytest.raises(nat.DcrxError) as e:      # 2^40 reads in all
        nat.downsample([0, 1], [1 << 39, 1 << 39], 2, [1, 1], 1)
    assert e.value.code == -2
    with pytest.raises(nat.DcrxError) as e:      # ... and a sum that would wrap
        nat.downsample([0, 0], [M, 2], 1, [1], 1)
    assert e.value.code == -2
    got = nat.downsample([], [], 3, [5, 0, M], 77)      # m = 0 touches no device
    assert [int(x) for x in got["threshold"]] == [M] * 3 and not got["reads"].any() and not got["depth_used"].any()
    assert len(got["kept"]) == 0
    with pytest.raises(nat.DcrxError) as e:
        nat.abundance_classes([0], [0], [1], 65)
    assert e.value.code == -1
    with pytest.raises(nat.DcrxError) as e:
        nat.abundance_classes([3], [0], [1], 3)
    assert e.value.code == -1
    with pytest.raises(nat.DcrxError) as e:
        nat.abundance_classes([0], [0], [1 << 32], 3)
    assert e.value.code == -2
    got = nat.abundance_classes([], [], [], 3)          # n = 0 touches no device
    assert [int(x) for x in got["class_off"]] == [0, 0, 0, 0] and len(got["class_count"]) == 0


# ---- the stage, with nat.* replaced by the Python contract ----

def write_inputs(tmp_path, tables):
    files = []
    for name, rows in tables:
        path = str(tmp_path / (name + ".clonotypes.tsv"))
        with open(path, "wb") as fh:
            fh.write(ou.clonotypes_text(rows))
        files.append(path)
    return files


def stage(tmp_path, monkeypatch, files, calls=None, **kw):
    monkeypatch.setattr(nat, "overlap", ou.brute_force_native())
    monkeypatch.setattr(nat, "downsample", ru.python_downsample(calls))
    monkeypatch.setattr(nat, "abundance_classes", ru.python_classes(calls))
    out = str(tmp_path / "out") + os.sep
    os.makedirs(out, exist_ok=True)
    inp = dict(command="overlap", infile=files, outpath=out, prefix="t_", dontgzip=True, overlap_key="vj", min_samples=2)
    inp.update(kw)
    res = ov.run(inp)
    read = lambda p: (gzip.open if p.endswith(".gz") else open)(p, "rb").read()
    return {k: read(res[k]) for k in ("pairs", "public", "diversity") if k in res}, res


def random_tables(seed=5, rows=(60, 25, 40)):
    rnd = np.random.default_rng(seed)
    keys = [(f"TRBV{k % 4}", f"TRBJ{k % 2}", "CASS" + ou.AMINO[k % 20] + ou.AMINO[k // 20 % 20] + "F") for k in range(70)]
    return [(name, [keys[int(rnd.integers(0, 70))] + (int(rnd.integers(1, 30)),) for _ in range(n)])
            for name, n in zip("ABC", rows)]


def kept_tables(tables, depth, seed):
    """The tables after the contract's subsample: what the stage must hand to the overlap call."""
    samples = [s for s, (_, rows) in enumerate(tables) for _ in rows]
    weights = [r[3] for _, rows in tables for r in rows]
    sub = ru.expected_downsample(samples, weights, len(tables), [depth] * len(tables), seed)
    kept = iter(int(x) for x in sub["kept"])
    out = []
    for name, rows in tables:
        out.append((name, [r[:3] + (k,) for r in rows for k in [next(kept)] if k]))
    return out, sub


def overlap_texts(tables, min_samples=2):
    """pairs and public text of tables by the overlap contract (tests/overlap_util.py), with the stage's class numbering."""
    samples = [s for s, (_, rows) in enumerate(tables) for _ in rows]
    rows = [r for _, t in tables for r in t]
    v, j, aa, w = ([r[k] for r in rows] for k in range(4))
    result, _ = ou.expected_overlap(samples, ou.call_classes(v, j, "vj"), aa, w, len(tables), min_samples)
    names = [name for name, _ in tables]
    return ov.pairs_text(names, result), ou.public_text(result, names, v, j, aa)


@pytest.mark.parametrize("depth", ["min", "200", "5000", "100000"])
def test_downsample_depths(tmp_path, monkeypatch, capsys, depth):
    tables = random_tables()
    reads = [sum(r[3] for r in rows) for _, rows in tables]
    assert min(reads) > 200 and max(reads) < 5000 and len(set(reads)) == 3
    calls = []
    texts, res = stage(tmp_path, monkeypatch, write_inputs(tmp_path, tables), calls, downsample=depth, seed=7)
    n = min(reads) if depth == "min" else int(depth)
    assert len(calls) == 1 and calls[0][0] == "downsample"      # ONE call, over the rows in file order, before any grouping
    assert calls[0][1] == [s for s, (_, rows) in enumerate(tables) for _ in rows] and calls[0][2] == [r[3] for _, t in tables for r in t]
    assert calls[0][3:] == (3, [n] * 3, 7)
    kept, sub = kept_tables(tables, n, 7)
    assert (texts["pairs"], texts["public"]) == overlap_texts(kept)      # the shared counts are those of the kept table
    assert res["downsample"]["depth_used"] == [min(n, x) for x in reads] and res["downsample"]["reads_in"] == reads
    assert res["downsample"]["rows_dropped"] == [len(rows) - len(k[1]) for (_, rows), k in zip(tables, kept)]
    out = capsys.readouterr().out
    assert f"Downsampled to {n:,} reads per sample (seed 7)" in out
    for (name, _), x in zip(tables, reads):      # a sample with fewer reads is kept whole, and a line says so
        assert (f"Sample {name} has {x:,} reads, fewer than {n:,}: it is kept whole" in out) == (x < n)
    pairs = [ln.split("\t") for ln in texts["pairs"].decode().splitlines()[1:]]
    assert [pairs[0][5], pairs[0][6], pairs[2][6]] == [str(min(n, x)) for x in reads]


def test_seed_changes_the_files_and_reproduces_them(tmp_path, monkeypatch):
    files = write_inputs(tmp_path, random_tables())
    a, _ = stage(tmp_path, monkeypatch, files, downsample="min", seed=1)
    b, _ = stage(tmp_path, monkeypatch, files, downsample="min", seed=2)
    c, _ = stage(tmp_path, monkeypatch, files, downsample="min", seed=1)
    d, res = stage(tmp_path, monkeypatch, files, downsample="min")
    assert a == c == d and a != b and res["downsample"]["seed"] == 1      # the default seed is 1


# Hand tables.  A: three clonotypes of 10, 5 and 1 reads (CASSA under two V calls is two clonotypes).  X = 16, R = 3, f1 = 1,
#   f2 = 0, largest 10; 2 * 10 >= 16: D50 = 1; Chao1 = 3 + 1 * 0 / 2 = 3; Simpson (90 + 20 + 0) / (16 * 15) = 110 / 240;
#   inverse Simpson 256 / (100 + 25 + 1) = 256 / 126; Gini, ascending 1, 5, 10 with 2 i - R - 1 = -2, 0, 2: 18 / (3 * 16);
#   Shannon (1/16) ln 16 + (5/16) ln (16/5) + (10/16) ln (16/10) = 0.173287 + 0.363485 + 0.293752 = 0.830524;
#   clonality 1 - 0.830524 / ln 3 = 0.244024.
# E: a header only.  O: one clonotype of one read.  M: two rows of one clonotype, 5 + 3 = 8 reads.
# D: clonotypes of 2, 2, 1, 1, 1, 4 reads.  X = 11, R = 6, f1 = 3, f2 = 2, largest 4; 4 + 2 = 6, 12 >= 11: D50 = 2;
#   Chao1 = 6 + 3 * 2 / (2 * 3) = 7; Simpson (2 + 2 + 12) / 110 = 16 / 110; inverse Simpson 121 / 27; Gini, ascending
#   1, 1, 1, 2, 2, 4 with -5, -3, -1, 1, 3, 5: (-9 + 2 + 6 + 20) / (6 * 11) = 19 / 66; Shannon 3 (1/11) ln 11 + 2 (2/11) ln 5.5
#   + (4/11) ln 2.75 = 0.653971 + 0.619908 + 0.367855 = 1.641734; clonality 1 - 1.641734 / ln 6 = 0.083731.
V, J = "TRBV1", "TRBJ1"
HAND = [("A", [(V, J, "CASSA", 10), (V, J, "CASSB", 5), ("TRBV2", J, "CASSA", 1)]),
        ("E", []),
        ("O", [(V, J, "CASSA", 1)]),
        ("M", [(V, J, "CASSQ", 5), (V, J, "CASSQ", 3)]),
        ("D", [(V, J, "CASSA", 2), (V, J, "CASSC", 2), (V, J, "CASSD", 1), (V, J, "CASSE", 1), (V, J, "CASSF", 1), (V, J, "CASSG", 4)])]
HAND_DIVERSITY = [
    ["A", "16", "16", "3", "1", "0", "10", "1", "3.000000", "0.458333", "2.031746", "0.375000", "0.830524", "0.244024"],
    ["E", "0", "0", "0", "0", "0", "0", "0", "0.000000", "nan", "nan", "nan", "0.000000", "nan"],
    ["O", "1", "1", "1", "1", "0", "1", "1", "1.000000", "nan", "1.000000", "0.000000", "0.000000", "nan"],
    ["M", "8", "8", "1", "0", "0", "8", "1", "1.000000", "1.000000", "1.000000", "0.000000", "0.000000", "nan"],
    ["D", "11", "11", "6", "3", "2", "4", "2", "7.000000", "0.145455", "4.481481", "0.287879", "1.641734", "0.083731"]]


def test_diversity_on_hand_tables(tmp_path, monkeypatch):
    calls = []
    texts, res = stage(tmp_path, monkeypatch, write_inputs(tmp_path, HAND), calls, diversity=True)
    assert os.path.basename(res["diversity"]) == "t_overlap_diversity.tsv" and oct(os.stat(res["diversity"]).st_mode)[-3:] == "666"
    ru.assert_diversity(texts["diversity"], HAND_DIVERSITY)
    assert [c[0] for c in calls] == ["abundance_classes"]      # no subsample without --downsample
    _, samples, groups, weights, S = calls[0]
    assert samples == [0, 0, 0, 2, 3, 3, 4, 4, 4, 4, 4, 4] and S == 5 and weights == [10, 5, 1, 1, 5, 3, 2, 2, 1, 1, 1, 4]
    assert groups == [int(g) for g in res["result"]["group_of"]]
    # ... and the same table from the raw cells, cell by cell
    ru.assert_diversity(texts["diversity"], ru.diversity_rows("AEOMD", [16, 0, 1, 8, 11], ru.cells_of(samples, groups, weights, 5)))


def test_diversity_after_downsampling(tmp_path, monkeypatch):
    tables = random_tables(seed=8, rows=(300, 120, 200))
    reads = [sum(r[3] for r in rows) for _, rows in tables]
    texts, res = stage(tmp_path, monkeypatch, write_inputs(tmp_path, tables), downsample="min", seed=3, diversity=True, dontgzip=False)
    assert res["diversity"].endswith("overlap_diversity.tsv.gz")
    kept, _ = kept_tables(tables, min(reads), 3)
    samples = [s for s, (_, rows) in enumerate(kept) for _ in rows]
    rows = [r for _, t in kept for r in t]
    groups = ou.call_classes([r[0] + "|" + r[2] for r in rows], [r[1] for r in rows], "vj")      # one number per (v, j, junction_aa)
    want = ru.diversity_rows("ABC", reads, ru.cells_of(samples, groups, [r[3] for r in rows], 3))
    ru.assert_diversity(texts["diversity"], want)
    assert [w[2] for w in want] == [str(min(reads))] * 3 and [w[1] for w in want] == [str(x) for x in reads]


def test_diversity_text_on_large_classes():
    """Classes with many clonotypes each: D50 inside a class, Gini over ranks that a class spans."""
    cells = [[1] * 1000 + [2] * 300 + [7] * 41 + [900, 900, 901]]
    classes = ru.expected_classes([0] * len(cells[0]), range(len(cells[0])), cells[0], 1)
    assert [int(x) for x in classes["class_mult"]] == [1000, 300, 41, 2, 1]
    ru.assert_diversity(ov.diversity_text(["s"], [5000], classes), ru.diversity_rows(["s"], [5000], cells))


def _no_open(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a file was opened before the refusal")
    monkeypatch.setattr(ov, "read_table", boom)
    for name in ("overlap", "downsample", "abundance_classes"):
        monkeypatch.setattr(nat, name, boom)


@pytest.mark.parametrize("kw,msg", [
    ({"downsample": "0"}, "--downsample"),
    ({"downsample": "-5"}, "--downsample"),
    ({"downsample": "1.5"}, "--downsample"),
    ({"downsample": "max"}, "--downsample"),
    ({"downsample": ""}, "--downsample"),
    ({"downsample": "10", "seed": -1}, "--seed"),
    ({"downsample": "min", "seed": 1 << 64}, "--seed"),
    ({"seed": 5}, "--seed"),
    ({"seed": 5, "diversity": True}, "--seed"),
])
def test_refusals_before_anything_is_opened(monkeypatch, kw, msg):
    _no_open(monkeypatch)
    inp = dict(command="overlap", infile=["a.clonotypes.tsv", "b.clonotypes.tsv"], outpath="", prefix="", dontgzip=True,
               overlap_key="vj", min_samples=2)
    inp.update(kw)
    assert msg in ov.refusal(inp)
    with pytest.raises(ValueError, match=msg):
        ov.run(inp)


def test_what_is_accepted():
    inp = dict(command="overlap", infile=["a.clonotypes.tsv"], min_samples=1)
    for kw in ({"downsample": "min"}, {"downsample": "1"}, {"downsample": 12, "seed": 0}, {"downsample": "7", "seed": (1 << 64) - 1},
               {"diversity": True}, {"downsample": None, "seed": None, "diversity": False}):
        assert ov.refusal(dict(inp, **kw)) is None


def test_refusal_from_the_command_line(monkeypatch, capsys):
    _no_open(monkeypatch)
    for argv, msg in ((["--seed", "3"], "--seed"), (["--downsample", "none"], "--downsample"), (["--downsample", "9", "--seed", "-2"], "--seed")):
        with pytest.raises(SystemExit) as e:
            pipeline.main(["overlap", "-in", "a.clonotypes.tsv", "b.clonotypes.tsv"] + argv)
        assert e.value.code == 2 and msg in capsys.readouterr().err


def test_all_samples_empty_with_min(tmp_path, monkeypatch):
    calls = []
    texts, res = stage(tmp_path, monkeypatch, write_inputs(tmp_path, [("E", []), ("F", [])]), calls, downsample="min", diversity=True)
    assert calls[0][4] == [0, 0] and res["downsample"]["depth"] == 0
    assert [ln.split("\t")[1:4] for ln in texts["diversity"].decode().splitlines()[1:]] == [["0", "0", "0"]] * 2


def test_without_the_flags_nothing_changes(tmp_path, monkeypatch, capsys):
    """No new native call, the two files and the printed lines as they were."""
    def boom(*a, **k):
        raise AssertionError("a new native entry was called without the flags")
    tables = random_tables()
    files = write_inputs(tmp_path, tables)
    monkeypatch.setattr(nat, "overlap", ou.brute_force_native())
    monkeypatch.setattr(nat, "downsample", boom)
    monkeypatch.setattr(nat, "abundance_classes", boom)
    out = str(tmp_path / "out") + os.sep
    os.makedirs(out)
    res = ov.run(dict(command="overlap", infile=files, outpath=out, prefix="t_", dontgzip=True, overlap_key="vj", min_samples=2))
    assert sorted(os.listdir(out)) == ["t_overlap_pairs.tsv", "t_overlap_public.tsv"] and "diversity" not in res and "downsample" not in res
    assert (open(res["pairs"], "rb").read(), open(res["public"], "rb").read()) == overlap_texts(tables)
    st = res["stats"]
    assert capsys.readouterr().out == (
        f"Overlap of 3 samples (vj): {st['rows_in']:,} rows in, {st['groups']:,} clonotypes, {st['private_groups']:,} "
        f"in one sample, {st['shared_groups']:,} in two or more, {st['in_all_samples']:,} in all (at most {st['largest_n_samples']} "
        f"samples hold one); {st['public_rows']:,} public rows with {st['public_cells']:,} cells\n")


def test_help_names_the_flags_and_the_others_are_unchanged():
    env = dict(os.environ, COLUMNS="100", PYTHONPATH=ROOT)
    run = lambda command: subprocess.run([sys.executable, "-m", "decombinator_amd", command, "--help"], capture_output=True, text=True,
                                         env=env, cwd=ROOT)
    got = run("overlap")
    assert got.returncode == 0 and all(flag in got.stdout for flag in ("--downsample", "--seed", "--diversity"))
    for command in ("decombine", "pipeline", "translate"):
        assert run(command).stdout.split() == open(os.path.join(HELP_DIR, command + ".txt")).read().split()
    from decombinator_amd.io import create_parser
    sub = [a for a in create_parser()._actions if getattr(a, "choices", None) and "overlap" in a.choices][0]
    assert list(sub.choices) == ["pipeline", "decombine", "collapse", "translate", "overlap"]      # flags of overlap: no new sub-command
