"""The error merge (`--merge-errors`) through the HIP path: dcrx_merge_dcrs and dcrx_merge_parents_device against the contract
written in Python (nm.expected_merge) — every array of the result, root_of and the statistics, exactly — on tables counted on
the GPU from noisy clonal reads, on one hot bucket, on degenerate tables, on lists constructed for the walk's decisions (decoys in
the bucket in front, both ends of the ratio prefix, tile and word edges, a chain of 384 links, 64-bit counts and ratios, the
primitive's out-of-reach rules and two calls on one work space), and the stage end to end against the oracle's DCRs put through
a Counter and expected_merge."""
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


# ---- constructed lists (tests/nbc_merge_util.py builds them and asserts each one's premise on the contract; their CPU twins
# are in test_nbc_merge.py): merge_parents_kernel's walk, the 64-bit counts, the primitive's rules.  What each list is there to
# fail: a walk that ignores `start` (1a, 1b) or stops after its first tile (1c at offset 256, 1e); `<=` for `<` at the prefix's
# end and `>` for `>=` at the early-out (1c); a distance that skips the second half (1f); needed_count without its overflow
# guard (2h); fewer than nine rounds of pointer jumping (1e); a bucket key without v (1b). ----

@pytest.fixture(scope="module")
def config2():
    ts = synth.config_tagset(2)
    return ts, _tables(ts)


@pytest.mark.parametrize("n_fill", nm.DECOY_FILLERS)
def test_padding_decoys_across_bucket_edges(config2, n_fill):
    """List 1a: X, X[:-1], X + "A" and X + "AA" pack to (nearly) the same dwords and stand in neighbouring buckets, which
    start at sorted position n_fill; only `p >= start` keeps a lane out of the bucket in front."""
    ts, t = config2
    for length in nm.DECOY_LENGTHS:
        for with_children in (False, True):
            counted, merges = nm.padding_decoys(ts, length, n_fill, with_children)
            assert _check(t, ts, counted, 2, 1)["merged"] == merges, (length, with_children)


@pytest.mark.parametrize("axis", ["v", "j"])
def test_identical_junction_under_another_gene_pair(config2, axis):
    """List 1b."""
    ts, t = config2
    counted = nm.gene_pair_decoys(ts, axis)
    for D, R in ((1, 10), (2, 1)):
        assert _check(t, ts, counted, D, R)["merged"] == (2 if R == 10 else 3)


@pytest.mark.parametrize("R", [1, 2, 10])
def test_prefix_ends(config2, R):
    """List 1c: the last eligible parent has exactly R * c reads (or one less, and then is none) at bucket offsets on and
    around a tile's edge and right in front of the child; offset 0 is the early-out's edge."""
    ts, t = config2
    for k, gap in nm.PREFIX_PLACES:
        for eligible in (True, False):
            counted, child, want = nm.prefix_end(ts, R, k, gap, eligible)
            for D in (1, 2):
                assert _check(t, ts, counted, D, R)["merged"] >= int(eligible), (k, gap, eligible, D)


@pytest.mark.parametrize("D", [1, 2])
def test_equal_counts_at_ratio_one(config2, D):
    """List 1d."""
    ts, t = config2
    assert _check(t, ts, nm.equal_counts_ball(ts), D, 1)["merged"] > 300


@pytest.mark.parametrize("n_out", [0, 200])
def test_deep_chain(config2, n_out):
    """List 1e: 384 links over two blocks; nine rounds of pointer jumping, and the depths add up."""
    ts, t = config2
    counted = nm.deep_chain(ts, n_out)
    for D in (1, 2):
        stats = _check(t, ts, counted, D, 1)
        assert stats["longest_chain"] == nm.CHAIN_LINKS // D and stats["roots_out"] == 1 + n_out and stats["reads_moved"] == 2688


def test_lengths_and_word_edges(config2):
    """List 1f."""
    ts, t = config2
    counted, expect = nm.lengths_and_word_edges(ts)
    for D in (1, 2):
        stats = _check(t, ts, counted, D, 10)
        assert stats["merged"] == 1 + sum(1 for _, nsub in expect.values() if nsub <= D) and stats["out_of_reach"] == 2
        _check(t, ts, counted, D, 1)


def test_short_and_unclean_windows():
    """List 1g: windows shorter than the anchor and an unclean one, through the device build of the tables."""
    from tests.test_nbc_merge import _short_region_tagset
    ts = _short_region_tagset()
    stats = _check(_tables(ts), ts, nm.short_window_mix(ts), 1, 10)
    assert stats["out_of_reach"] == 4 and stats["merged"] == 7


def test_counts_and_ratios_up_to_64_bits(config2):
    """List 2h."""
    ts, t = config2
    for name, counted, D, R, roots in nm.big_counts(ts):
        got, stats, root_of = nat.merge_dcrs(t, counted, D, R)
        assert root_of.tolist() == roots, name
        _check(t, ts, counted, D, R)


def test_a_count_of_zero_is_a_child(config2):
    """List 2i."""
    ts, t = config2
    for D, R in ((1, 10), (2, 1), (1, nm.U64)):
        assert _check(t, ts, nm.zero_counts(ts), D, R)["merged"] == 1


class _DeviceTable:
    """A counted table in device memory, as dcrx_merge_parents_device takes it."""

    def __init__(self, counted, text_bytes=None):
        self.n = len(counted["v"])
        self.bufs = [nat.DeviceBuffer.from_host(np.ascontiguousarray(counted[f], dtype=ty))
                     for f, ty in (("v", np.uint16), ("j", np.uint16), ("vdel", np.uint8), ("jdel", np.uint8), ("count", np.uint64),
                                   ("ins_off", np.uint64))]
        text = np.frombuffer(counted["ins_text"], np.uint8)
        self.text = nat.DeviceBuffer.from_host(text)
        self.text_bytes = len(text) if text_bytes is None else text_bytes
        self.parent, self.reach = nat.DeviceBuffer(4 * self.n), nat.DeviceBuffer.from_host(np.full(self.n, 7, np.uint8))

    def launch(self, t, D, R, work, work_bytes, stream, parent=None, with_reach=True):
        nat.merge_parents_device(t, self.n, *self.bufs, self.text, self.text_bytes, D, R, parent or self.parent,
                                 self.reach if with_reach else None, work, work_bytes, stream.ptr)


def test_primitive_out_of_reach_rules(config2):
    """List 2j: a v or j the tables do not have and inserts that leave the text or go backwards are out of reach, nothing
    more: reach is 0 exactly there, such an entry is its own parent and no one else's, the rest is the contract's."""
    ts, t = config2
    dev, contract, bad = nm.primitive_defects(ts)
    d = _DeviceTable(dev, dev["text_bytes"])
    wb = int(nat.lib().dcrx_merge_work_bytes(d.n))
    work, s = nat.DeviceBuffer(wb), nat.Stream()
    for D, R in ((1, 10), (2, 1)):
        d.launch(t, D, R, work, wb, s)
        s.synchronize()
        want_parent, want_reach = nm.expected_parents(contract, ts, D, R)
        reach = d.reach.to_host(np.uint8, d.n)
        assert np.nonzero(reach == 0)[0].tolist() == bad and set(reach.tolist()) == {0, 1}
        assert reach.astype(bool).tolist() == want_reach
        parent = d.parent.to_host(np.uint32, d.n)
        assert parent.tolist() == want_parent and all(parent[k] == k for k in bad)


def test_two_calls_in_a_row_share_a_work_space(config2):
    """List 2k: calls back to back on one stream of the caller's, one work space, no synchronisation in between, each into
    its own parent buffer; one of them without reach flags."""
    ts, t = config2
    a = nm.padding_decoys(ts, 64, 255, True)[0]
    b = nm.equal_counts_ball(ts)
    da, db = _DeviceTable(a), _DeviceTable(b)
    wb = max(int(nat.lib().dcrx_merge_work_bytes(x.n)) for x in (da, db))
    work, s = nat.DeviceBuffer(wb), nat.Stream()
    calls = [(da, 2, 1, True), (db, 1, 1, False), (da, 1, 1, False), (db, 2, 1, True)]
    single = []
    for d, D, R, with_reach in calls:          # one call at a time
        d.launch(t, D, R, work, wb, s, with_reach=with_reach)
        s.synchronize()
        single.append(d.parent.to_host(np.uint32, d.n))
        want_parent, want_reach = nm.expected_parents(a if d is da else b, ts, D, R)
        assert single[-1].tolist() == want_parent
        assert d.reach.to_host(np.uint8, d.n).tolist() == ([int(x) for x in want_reach] if with_reach else [7] * d.n)
        d.reach = nat.DeviceBuffer.from_host(np.full(d.n, 7, np.uint8))
    outs = [nat.DeviceBuffer.from_host(np.full(d.n, 0xFFFFFFFF, np.uint32)) for d, _, _, _ in calls]
    for (d, D, R, with_reach), out in zip(calls, outs):          # all four in a row
        d.launch(t, D, R, work, wb, s, parent=out, with_reach=with_reach)
    s.synchronize()
    for (d, _, _, _), out, want in zip(calls, outs, single):
        assert np.array_equal(out.to_host(np.uint32, d.n), want)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_work_space_of_exactly_the_bytes_asked_for(config2, n):
    ts, t = config2
    counted = nm.take(nm.equal_counts_ball(ts), n)
    d = _DeviceTable(counted)
    wb = int(nat.lib().dcrx_merge_work_bytes(n))
    assert wb > 256
    work, s = nat.DeviceBuffer(wb), nat.Stream()
    d.launch(t, 2, 1, work, wb, s)
    s.synchronize()
    assert d.parent.to_host(np.uint32, n).tolist() == nm.expected_parents(counted, ts, 2, 1)[0]
    with pytest.raises(nat.DcrxError, match="work space"):
        d.launch(t, 2, 1, work, wb - 256, s)


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
