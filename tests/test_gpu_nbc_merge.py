"""The error merge (`--merge-errors`) through the HIP path: dcrx_merge_dcrs and dcrx_merge_parents_device against the contract
written in Python (nm.expected_merge) — every array of the result, root_of and the statistics, exactly — on tables counted on
the GPU from noisy clonal reads, on one hot bucket, on degenerate tables, and the stage end to end against the oracle's DCRs put
through a Counter and expected_merge."""
import gzip

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import decombine as dec
from decombinator_amd import pipeline, synth
from tests import nbc_count_util as nu
from tests import nbc_merge_util as nm

pytestmark = pytest.mark.gpu


def _tables(ts):
    return nat.Tables(ts.v_tags, ts.v_jumps, ts.v_regions, ts.j_tags, ts.j_jumps, ts.j_regions, *ts.half_splits)


def _check(t, ts, counted, D, R):
    got, stats, root_of = nat.merge_dcrs(t, counted, D, R)
    want, wstats, wroot = nm.expected_merge(counted, ts, D, R)
    assert stats == wstats
    assert np.array_equal(root_of, wroot)
    nm.same_table(got, want)
    assert int(got["count"].sum()) == int(counted["count"].sum())
    return stats


@pytest.mark.parametrize("orientation", ["reverse", "both"])
def test_noisy_clonal_table(orientation):
    ts = synth.config_tagset(2)
    t = _tables(ts)
    reads = nm.noisy_clonal_reads(ts, 2_000_000, seed=91, n_pool=3000, zipf=1.1, sub_rate=0.005, orientation=orientation)[0]
    dc = nat.DcrCounts()
    cnt = nat.decombine_count(t, nat.pack_reads(reads), dc, 0, None, orientation)
    counted = dc.read()
    dc.close()
    assert int(counted["count"].sum()) == int(cnt[19]) and len(counted["v"]) > 50_000
    assert nm.out_of_reach_share(counted, ts) <= 0.01
    for D, R in ((1, 10), (2, 3)):
        stats = _check(t, ts, counted, D, R)
        assert stats["merged"] > 20_000 and stats["longest_chain"] >= 2


def test_config3_pair_through_the_chains_entry():
    ta, tb = synth.config3_tagsets()
    tables = [_tables(ta), _tables(tb)]
    reads = nm.noisy_clonal_reads(ta, 500_000, seed=93, n_pool=1500, zipf=1.1)[0] + \
        nm.noisy_clonal_reads(tb, 500_000, seed=94, n_pool=1500, zipf=1.1)[0]
    np.random.default_rng(4).shuffle(reads)
    dcs = [nat.DcrCounts(), nat.DcrCounts()]
    nat.decombine_chains_count(tables, nat.pack_reads(reads), dcs, 0)
    for t, ts, dc in zip(tables, (ta, tb), dcs):
        counted = dc.read()
        dc.close()
        assert nm.out_of_reach_share(counted, ts) <= 0.01
        assert _check(t, ts, counted, 1, 10)["merged"] > 5_000


def _hot_bucket(ts, n_top=3000, n_low=20_000, seed=5):
    """One (v, j, length): n_top abundant entries (random 24-base inserts, counts 100 000 down to 1 000) and n_low entries of
    count 1 .. 60, a third of them one substitution from an abundant entry — many from the LAST abundant entries, so that
    their parent sits in the last tile of a prefix that crosses a dozen tiles."""
    rng = np.random.default_rng(seed)
    tops = ["".join(rng.choice(list("ACGT"), size=24)) for _ in range(n_top)]
    entries = [(1, 2, 4, 3, s, int(100_000 - k * 33), k) for k, s in enumerate(tops)]
    seen = set(tops)
    for k in range(n_low):
        kind = k % 3
        if kind == 0:
            src = tops[n_top - 1 - int(rng.integers(0, 200))] if k % 2 else tops[int(rng.integers(0, n_top))]
            p = int(rng.integers(0, 24))
            s = src[:p] + "ACGT"[("ACGT".index(src[p]) + int(rng.integers(1, 4))) % 4] + src[p + 1:]
        else:
            s = "".join(rng.choice(list("ACGT"), size=24))
        if s in seen:
            continue
        seen.add(s)
        entries.append((1, 2, 4, 3, s, int(rng.integers(1, 61)), n_top + k))
    return nm.ranked(entries)


def test_one_hot_bucket():
    ts = synth.config_tagset(2)
    t = _tables(ts)
    counted = _hot_bucket(ts)
    assert len(counted["v"]) > 22_000
    stats = _check(t, ts, counted, 1, 10)
    assert stats["merged"] > 5_000 and stats["out_of_reach"] == 0
    want_root = nm.expected_merge(counted, ts, 1, 10)[2]
    merged = np.nonzero(want_root != np.arange(len(want_root)))[0]
    # children far down the table whose parent is among the last abundant entries
    assert ((want_root[merged] > 2800) & (merged > 15_000)).sum() > 100
    _check(t, ts, counted, 2, 1)


def test_degenerate_tables():
    ts = synth.config_tagset(2)
    t = _tables(ts)
    A = "ACGTTGCAAGGT"
    sub = A[:3] + "A" + A[4:]
    _check(t, ts, nm.table([]), 1, 10)
    _check(t, ts, nm.table([(0, 0, 1, 1, A, 7, 0)]), 1, 10)
    assert _check(t, ts, nm.table([(0, 0, 1, 1, A, 70, 0), (0, 0, 1, 1, sub, 7, 1)]), 1, 10)["merged"] == 1
    assert _check(t, ts, nm.table([(0, 0, 1, 1, A, 69, 0), (0, 0, 1, 1, sub, 7, 1)]), 1, 10)["merged"] == 0
    # every entry out of reach
    rng = np.random.default_rng(2)
    out = [(int(rng.integers(0, 4)), int(rng.integers(0, 4)), 2, 2, "".join(rng.choice(list("ACGT"), size=10)) + "N", int(1000 - k), k)
           for k in range(700)]
    stats = _check(t, ts, nm.table(out), 1, 1)
    assert stats["out_of_reach"] == 700 and stats["merged"] == 0
    # no merges: far apart, or too close in count
    far = nm.ranked([(int(k % 3), 1, 2, 2, "".join(rng.choice(list("ACGT"), size=30)), int(rng.integers(1, 9)), k) for k in range(5000)])
    assert _check(t, ts, far, 2, 10)["merged"] == 0
    # lower-case and IUPAC inserts, and deletions beyond the anchor, beside entries in reach
    mix = nm.ranked([(0, 0, 1, 1, A, 500, 0), (0, 0, 1, 1, sub, 5, 1), (0, 0, 1, 1, sub.lower(), 5, 2), (0, 0, 33, 1, A, 4, 3),
                     (0, 0, 1, 1, A[:5] + "R" + A[6:], 3, 4), (0, 0, 1, 1, "ACGT" * 32, 2, 5)])
    stats = _check(t, ts, mix, 1, 10)
    assert stats["out_of_reach"] == 4 and stats["merged"] == 1


def _paired_bucket(n, equal_totals, seed=21):
    """n entries of one (v, j, length) bucket in rank order (nm.ranked), and the mask of the intended children: pairs of a parent
    and a child one substitution from it with at least ten times fewer reads, the other inserts far apart, first ordinals a
    permutation that has nothing to do with the ranks.  With equal_totals every root ends with the same total: the parents
    (and, for an odd n, one entry that stands alone) fill the first ranks and every child stands behind every root — a child
    has at most a tenth of its parent's reads, so equal totals and children between the roots exclude each other.  Without
    it there are two totals (11 000 and 800: the lesser pairs' parents have as many reads as the greater pairs' children, so
    roots and children alternate over the middle half of the table) and, for an odd n, a last entry of one read that stands
    alone: the table's last rank is then a root, in a block of its own at 257 and 513."""
    rng = np.random.default_rng(seed + n)
    pairs = n // 2
    greater = pairs if equal_totals else pairs // 2
    first = rng.permutation(n).tolist()
    entries, child_of, seen = [], {}, set()

    def insert():
        while True:
            s = "".join(rng.choice(list("ACGT"), size=24))
            if s not in seen:
                seen.add(s)
                return s
    for k in range(pairs):
        total, y = (11_000, int(rng.integers(730, 800))) if k < greater else (800, int(rng.integers(2, 72)))
        src = insert()
        p = int(rng.integers(0, 24))
        sub = src[:p] + "ACGT"[("ACGT".index(src[p]) + int(rng.integers(1, 4))) % 4] + src[p + 1:]
        seen.add(sub)
        entries += [(1, 2, 4, 3, src, total - y, first.pop()), (1, 2, 4, 3, sub, y, first.pop())]
        child_of[sub] = src
    if n % 2:
        entries.append((1, 2, 4, 3, insert(), 11_000 if equal_totals else 1, first.pop()))
    counted = nm.ranked(entries)
    return counted, np.array([x in child_of for x in nm.inserts(counted)])


@pytest.mark.parametrize("equal_totals", [True, False], ids=["equal-totals", "interleaved"])
@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_tables_on_a_block_edge(n, equal_totals):
    """Tables that end on, one before and one behind a block of 256, and in a third block: the roots' compaction, its count and
    the order of roots whose totals tie (the first ordinal decides).  Equal totals and children between the roots exclude
    each other (_paired_bucket), so each has a table of its own."""
    ts = synth.config_tagset(2)
    counted, child = _paired_bucket(n, equal_totals)
    want, wstats, wroot = nm.expected_merge(counted, ts, 1, 10)
    is_root = wroot == np.arange(n)
    assert np.array_equal(~is_root, child) and wstats["merged"] == n // 2 and wstats["out_of_reach"] == 0
    assert (np.bincount(wroot[child], minlength=n) <= 1).all()          # every parent has exactly one child
    totals = set(want["count"].tolist())
    assert totals == ({11_000} if equal_totals else {11_000, 800, 1} if n % 2 else {11_000, 800})
    if not equal_totals:
        edge = min(256, n - 1)          # (the last block's first entry; in a table of one block, its last)
        assert child[:edge].any() and is_root[:edge].any() and is_root[n - 1] == n % 2
        if n > 256:          # a root and a child on either side of index 256 (257 has one entry there: the root that stands alone)
            assert is_root[256:].any() and (child[256:].any() or n == 257)
        mixed = np.nonzero(child[:-1] != child[1:])[0]
        assert len(mixed) > n // 8 and (n < 513 or (mixed.min() < 256 < mixed.max()))
    _check(_tables(ts), ts, counted, 1, 10)


def test_parents_device_on_a_stream_of_the_callers():
    ts = synth.config_tagset(2)
    t = _tables(ts)
    reads = nm.noisy_clonal_reads(ts, 300_000, seed=95, n_pool=800, zipf=1.1)[0]
    dc = nat.DcrCounts()
    nat.decombine_count(t, nat.pack_reads(reads), dc)
    counted = dc.read()
    dc.close()
    n = len(counted["v"])
    want_root = nm.expected_merge(counted, ts, 1, 10)[2]
    bufs = [nat.DeviceBuffer.from_host(counted[f]) for f in ("v", "j", "vdel", "jdel", "count", "ins_off")]
    text = np.frombuffer(counted["ins_text"], np.uint8)
    d_text = nat.DeviceBuffer.from_host(text)
    work_bytes = int(nat.lib().dcrx_merge_work_bytes(n))
    assert work_bytes > 0
    d_work, d_parent, d_reach = nat.DeviceBuffer(work_bytes), nat.DeviceBuffer(4 * n), nat.DeviceBuffer(n)
    s = nat.Stream()
    nat.merge_parents_device(t, n, *bufs, d_text, len(text), 1, 10, d_parent, d_reach, d_work, work_bytes, s.ptr)
    s.synchronize()
    parent = d_parent.to_host(np.uint32, n)
    assert (parent <= np.arange(n)).all()
    assert np.array_equal(nm.roots_of(parent), want_root)
    assert d_reach.to_host(np.uint8, n).all()
    # too small a work space is an error, not a launch
    with pytest.raises(nat.DcrxError, match="work space"):
        nat.merge_parents_device(t, n, *bufs, d_text, len(text), 1, 10, d_parent, d_reach, d_work, work_bytes - 256, s.ptr)


def _merges_text(counted, root_of):
    rows = nat.count_rows(counted)
    return "".join(", ".join(rows[k][:5] + [str(rows[k][5])] + rows[int(root_of[k])][:5]) + "\n"
                   for k in range(len(rows)) if root_of[k] != k)


def _read(p):
    return (gzip.open(p).read() if str(p).endswith(".gz") else p.read_bytes()).decode("latin-1")


@pytest.mark.parametrize("command,gz", [("decombine", False), ("pipeline", True)])
def test_stage_end_to_end(command, gz, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(dec, "BATCH_READS", 8192)
    if command == "pipeline":
        from tests.test_nbc_count import _translate_stubs
        _translate_stubs(monkeypatch)
    ts = synth.config_tagset(2)
    reads = nm.noisy_clonal_reads(ts, 40_000, seed=97, n_pool=300, orientation="both")[0]
    argv = nu.workdir_with(tmp_path, ts, reads) + ["--merge-errors", "--write-merges", "-or", "both"] + ([] if gz else ["-dz"])
    pipeline.main([command] + argv)
    keys, _ = nu.read_dcrs(nu.oracle_for(ts), reads, "both")
    counted = nm.counted_from_keys(keys)
    want, stats, root_of = nm.expected_merge(counted, ts, 1, 10)
    end = ".gz" if gz else ""
    assert _read(tmp_path / f"dcr_NBC_1_beta.nbc{end}") == nu.counted_text(want)
    assert _read(tmp_path / f"dcr_NBC_1_beta.merges{end}") == _merges_text(counted, root_of)
    assert dec.merge_stats == stats and stats["merged"] > 500
    assert nm.out_of_reach_share(counted, ts) <= 0.01
    assert int(want["count"].sum()) == dec.counts["vj_count"]


def test_stage_both_chains(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ta, tb = synth.config3_tagsets()
    reads = nm.noisy_clonal_reads(ta, 20_000, seed=98, n_pool=200)[0] + nm.noisy_clonal_reads(tb, 20_000, seed=99, n_pool=200)[0]
    np.random.default_rng(6).shuffle(reads)
    ta.write(str(tmp_path / "tags"))
    tb.write(str(tmp_path / "tags"))
    nu.write_fastq(tmp_path / "NBC_1.fq", reads)
    pipeline.main(["decombine", "-in", "NBC_1.fq", "-br", "R2", "-nbc", "--count-dcrs", "--merge-errors", "--write-merges", "--merge-distance",
                   "2", "--merge-ratio", "5", "-tfdir", "tags", "-tg", ta.tags, "-sp", ta.species, "-dc", "-dz", "-c", f"{ta.chain},{tb.chain}"])
    for ts in (ta, tb):
        keys, _ = nu.read_dcrs(nu.oracle_for(ts), reads)
        counted = nm.counted_from_keys(keys)
        want, stats, root_of = nm.expected_merge(counted, ts, 2, 5)
        name = f"dcr_NBC_1_{dec.chainnams[ts.chain]}"
        assert (tmp_path / f"{name}.nbc").read_text() == nu.counted_text(want)
        assert (tmp_path / f"{name}.merges").read_text() == _merges_text(counted, root_of)
        assert dec.chain_merge_stats[ts.chain] == stats and stats["merged"] > 200
