"""The CDR3 network's Levenshtein metric (`--cdr3-network --cdr3-metric levenshtein`) through the HIP path:
dcrx_cdr3_network_metric against the contract written in Python (clu.expected_lev_network: symmetric deletion, a plain DP,
union-find) — degree, the CSR adjacency, cluster_of, the cluster rows and the statistics, exactly, with and without the edges
— on degenerate inputs, every edit position, raw bytes, classes across tiles and blocks, long components and random families
with indels; the primitive's work space and adjacency rules; and the stage end to end."""
import ctypes as C
import gzip
import json
import random

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import pipeline, synth
from tests import cdr3_lev_util as clu
from tests import cdr3_network_util as cnu
from tests import clonotype_util as cu

pytestmark = pytest.mark.gpu
LEV = "levenshtein"


def _run(classes, strings, D, weights=None, want_edges=True):
    off, text = cnu.node_text(strings)
    w = [1 + (7 * k) % 13 for k in range(len(strings))] if weights is None else weights
    return nat.cdr3_network(classes, off, text, w, D, want_edges=want_edges, metric=LEV), w


def _check(classes, strings, D, weights=None, want=None):
    """The native result with edges (and the one without) against the contract; returns the expected (result, stats)."""
    got, w = _run(classes, strings, D, weights)
    if want is None:
        want = clu.expected_lev_network(classes, strings, w, D)
    cnu.assert_same(got, want)
    plain, _ = _run(classes, strings, D, w, want_edges=False)
    assert "adj" not in plain[0]
    cnu.assert_same(plain, want)
    return want


# ---- degenerate inputs ----

@pytest.mark.parametrize("D", [1, 2])
def test_no_node_one_node_two_nodes(D):
    _check([], [], D)
    assert _check([7], ["CASSF"], D)[1]["clusters_out"] == 1
    assert _check([0, 0], ["CASSF", "CASSFF"], D)[1]["edges"] == 1
    assert _check([0, 0], ["CASSF", "CASSFFF"], D)[1]["edges"] == (1 if D == 2 else 0)
    assert _check([0, 1], ["CASSF", "CASSFF"], D)[1]["edges"] == 0
    assert _check([0, 1, 0, 1], ["CASSF", "CASSFF", "CASSFF", "CASSF"], D)[1]["edges"] == 2
    assert _check([0, 0], ["A", "AC"], D)[1]["edges"] == 1
    assert _check([0, 0], ["CASSF", "CASSY"], D)[1]["edges"] == 1
    _, st = _check([0, 0], ["A" * 32, "A" * 33], D)
    assert st["edges"] == 0 and st["out_of_reach"] == 1
    assert _check([0, 0], ["A" * 32, "A" * 31], D)[1]["edges"] == 1


def test_every_node_out_of_reach():
    strings = ["", "A" * 33, "", "C" * 40, "A" * 33] * 70
    _, st = _check([0] * len(strings), strings, 1)
    assert st["out_of_reach"] == st["clusters_out"] == st["singletons"] == 350 and st["edges"] == 0


# ---- every edit position ----

@pytest.mark.parametrize("D", [1, 2])
def test_every_edit_position(D):
    """Per length a base of distinct-enough letters, every single deletion, every insertion (where the result still fits) and
    pairs of edits at the dword edges, all lengths in one class, ranks shuffled."""
    rnd = random.Random(100 + D)
    strings = []
    for L in (1, 2, 4, 5, 8, 9, 16, 17, 31, 32):
        base = "".join(rnd.choice(cnu.AMINO) for _ in range(L))
        strings.append(base)
        strings += [base[:p] + base[p + 1:] for p in range(L) if L > 1]
        if L + 1 <= 32:
            strings += [base[:p] + rnd.choice(cnu.AMINO) + base[p:] for p in range(L + 1)]
        spots = sorted({p for p in (0, 3, 4, 7, 8, L - 4, L - 1) if 0 <= p < L})
        for p in spots:
            for q in spots:
                if p < q:
                    sub = base[:p] + "X" + base[p + 1:]
                    strings.append(sub[:q] + sub[q + 1:])                                   # a substitution and a deletion
                    if L > 2:
                        strings.append(base[:p] + base[p + 1:q] + base[q + 1:])             # two deletions
                    if L + 1 <= 32:
                        strings.append(base[:p] + "X" + base[p:q] + base[q + 1:])           # an insertion and a deletion
    rnd.shuffle(strings)
    (r, st) = _check([0] * len(strings), strings, D)
    two, extra = clu.edge_kinds(strings, r, D)
    assert st["edges"] > 300 and two > 200 and st["out_of_reach"] == 0 and (D == 1 or extra > 0)


def test_a_rotation_is_two_edits():
    s = "ACDEFGHIKLMN"
    strings = [s, s[1:] + s[0], s[-1] + s[:-1], s]
    assert _check([0] * 4, strings, 1)[1]["edges"] == 1          # (only the twins)
    r, st = _check([0] * 4, strings, 2)
    assert st["edges"] == 5 and r["degree"].tolist() == [3, 2, 2, 3]      # (the two rotations are four edits apart)


def test_runs_of_one_letter():
    strings = ["A" * k for k in range(1, 33)]
    random.Random(3).shuffle(strings)
    _, st = _check([0] * 32, strings, 1)
    assert st["edges"] == 31 and st["clusters_out"] == 1 and st["largest_degree"] == 2
    _, st = _check([0] * 32, strings, 2)
    assert st["edges"] == 61 and st["largest_degree"] == 4


def test_bytes_are_compared_as_they_are():
    base = [b"CASSLGQAYEQYF", b"CASSL\x00QAYEQYF", b"CASSL\x7fQAYEQYF", b"CASSL\x80QAYEQYF", b"CASSL\xffQAYEQYF", b"CASSLgQAYEQYF",
            b"CASSL\x27QAYEQYF", b"CASSLQAYEQYF", b"CASSLG\x00QAYEQYF", b"\xff" * 32, b"\x7f" + b"\xff" * 31, b"\xff" * 31, b"\x00" * 32,
            b"\x00" * 31 + b"\x80", b"\x00" * 30, b"\x00", b"\x00\x00", b"CASS\x00", b"CASS", b"A!a\x01\x21\x41\x61\x81", b"A!a\x01\x21\x41\x61",
            b"!a\x01\x21\x41\x61\x81", b"casslgqayeqyf"]
    strings = base + base                   # the same strings in two classes
    classes = [0] * len(base) + [1] * len(base)
    for D in (1, 2):
        r, st = _check(classes, strings, D)
        assert st["edges"] % 2 == 0 and int(r["degree"][len(base) - 1]) == 0      # lower case is another string
        near = r["adj"][int(r["adj_off"][17]):int(r["adj_off"][18])].tolist()      # b"CASS\x00"
        assert 18 in near and not set(near) & set(range(len(base), 2 * len(base)))
        assert 16 in r["adj"][int(r["adj_off"][15]):int(r["adj_off"][16])].tolist()      # one and two zero bytes
    both, _ = _check([0] * len(strings), strings, 1)      # under one class every string meets its twin at distance 0
    assert int(both["degree"][len(base) - 1]) == 1


# ---- classes against tiles and blocks ----

@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_one_class_across_tile_boundaries(n):
    strings = clu.families_indel(n, seed=n, length=12)
    D = 1 + n % 2
    r, st = _check([0] * n, strings, D)
    assert st["edges"] > n // 4 and st["out_of_reach"] == 0 and clu.edge_kinds(strings, r, D)[0] > n // 10


def test_many_small_classes_in_one_block():
    rnd = random.Random(21)
    nodes, cls = [], 0
    while len(nodes) < 600:
        seed = "".join(rnd.choice(cnu.AMINO) for _ in range(14))
        for _ in range(min(1 + cls % 7, 600 - len(nodes))):
            nodes.append((cls, clu.edit(seed, rnd.randrange(0, 3), rnd)))
        cls += 1
    rnd.shuffle(nodes)
    for D in (1, 2):
        _, st = _check([c for c, _ in nodes], [s for _, s in nodes], D)
        assert st["edges"] > 100 and st["clusters_out"] >= cls


def test_a_class_that_starts_at_the_last_lane_of_a_block():
    strings = clu.families_indel(255, seed=5, length=10) + clu.families_indel(300, seed=6, length=10)
    classes = [0] * 255 + [1] * 300        # class 1 starts at sorted position 255
    _, st = _check(classes, strings, 2)
    assert st["edges"] > 200
    # ... and with nodes out of reach in front in rank order (they sort behind every class)
    _check([0] * 50 + classes, [""] * 25 + ["A" * 33] * 25 + strings, 1)


# ---- decoys: equal packed words at neighbouring lengths, classes that differ in their high bits ----

@pytest.mark.parametrize("D", [1, 2])
def test_a_zero_byte_is_one_insertion(D):
    """b"CASSF", b"CASSF\\0" and b"CASSF\\0\\0" (and a pair of 31 and 32 bytes) pack to the same dwords: the edges are exactly the
    length steps, one apart at D = 1 and also two apart at D = 2.  The run straddles sorted position 256."""
    classes, strings, at = cnu.zero_byte_run(clu.families_indel(cnu.ZERO_RUN_FRONT, seed=41, length=6))
    r, st = _check(classes, strings, D)
    near = [sorted(int(x) - at for x in r["adj"][int(r["adj_off"][k]):int(r["adj_off"][k + 1])]) for k in range(at, at + 6)]
    assert near == ([[1, 5], [0, 2], [1], [4], [3], [0]] if D == 1 else [[1, 2, 5], [0, 2, 5], [0, 1], [4], [3], [0, 1]])
    assert cnu.no_edge_across(classes, r)


@pytest.mark.parametrize("pair", cnu.CLASS_BIT_PAIRS, ids=["bit31", "bit26", "all-ones"])
def test_classes_that_differ_in_their_high_bits(pair):
    """As in test_gpu_cdr3_network.py, under the Levenshtein metric (the bucket is the class alone)."""
    classes, strings, plain = cnu.class_bit_nodes(clu.families_indel(150, seed=43, length=12), pair, n_out=40 if pair[1] == 0xFFFFFFFF else 0)
    w = [1 + (7 * k) % 13 for k in range(len(strings))]
    for D in (1, 2):
        want = _check(classes, strings, D)
        cnu.assert_same(want, clu.expected_lev_network(plain, strings, w, D))
        assert want[1]["edges"] > 100 and cnu.no_edge_across(classes, want[0])


# ---- component rounds ----

def test_a_shuffled_path_grown_letter_by_letter():
    rnd = random.Random(8)
    chain = ["".join(cnu.AMINO[(3 * k) % 20] for k in range(n)) for n in range(1, 33)]
    order = list(range(32))
    rnd.shuffle(order)
    strings = [None] * 32
    for t, r in enumerate(order):
        strings[r] = chain[t]
    r, st = _check([0] * 32, strings, 1)
    assert st["clusters_out"] == 1 and st["edges"] == 31 and st["largest_degree"] == 2


def test_a_star_of_deletions_and_insertions_adds_onto_one_head():
    centre = "ACDEFGHIKLMNPQRSTVWY"
    leaves = [centre[:p] + centre[p + 1:] for p in range(20)] + [centre[:p] + "X" + centre[p:] for p in range(21)]
    strings = leaves[:17] + [centre] + leaves[17:]
    r, st = _check([0] * 42, strings, 1, weights=[1 << 40] * 42)
    assert st["clusters_out"] == 1 and int(r["degree"][17]) == 41 and int(r["cluster_weight"][0]) == 42 << 40


# ---- random families ----

@pytest.fixture(scope="module")
def family_strings():
    return clu.families_indel(20000, seed=7)


@pytest.mark.parametrize("n_classes", [1, 16])
def test_random_families_at_one_edit(family_strings, n_classes):
    """clu.families_indel(20000, seed=7): 20-letter seeds, each with a family of 3 to 10 strings 1 to 3 edits away.  With 16
    classes a node's class is its first letter's number modulo 16."""
    n = len(family_strings)
    classes = [0 if n_classes == 1 else cnu.AMINO.index(x[0]) % n_classes for x in family_strings]
    r, st = _check(classes, family_strings, 1)
    assert st["edges"] >= n // 2 and clu.edge_kinds(family_strings, r, 1)[0] >= n // 4      # (no degenerate input passes for a result)


def test_random_families_at_two_edits():
    """clu.families_indel(5000, seed=7) under one class (the brute force takes tens of seconds on the 20 000-node table)."""
    strings = clu.families_indel(5000, seed=7)
    n = len(strings)
    r, st = _check([0] * n, strings, 2)
    two, extra = clu.edge_kinds(strings, r, 2)
    assert st["edges"] >= n and two >= n // 2 and extra >= n // 10


# ---- the primitive ----

def _primitive(classes, strings, D, metric=LEV, work_bytes=None, adj_cap=None, pattern=0xA5):
    """dcrx_cdr3_neighbours_metric_device over buffers and a stream of the caller's: (degree, adj_off, the whole adj buffer,
    need, cap)."""
    m = len(strings)
    off, text = cnu.node_text(strings)
    d_cls = nat.DeviceBuffer.from_host(np.asarray(classes, dtype=np.uint32))
    d_off = nat.DeviceBuffer.from_host(off)
    d_text = nat.DeviceBuffer.from_host(np.frombuffer(text + b"\0", np.uint8))
    d_deg, d_adj_off, d_need = nat.DeviceBuffer(max(16, m * 4)), nat.DeviceBuffer((m + 1) * 8), nat.DeviceBuffer(16)
    wb = nat.cdr3net_work_bytes(m, len(text), metric=metric) if work_bytes is None else work_bytes
    assert wb > m * 32 or work_bytes is not None
    d_work = nat.DeviceBuffer(max(256, wb))
    stream = C.c_void_p()
    nat.check(nat.lib().dcrx_stream_create(C.byref(stream)))
    try:
        nat.cdr3_neighbours_device(m, d_cls, d_off, d_text, len(text), D, d_deg, d_adj_off, None, 0, d_need, d_work, wb, stream, metric=metric)
        nat.check(nat.lib().dcrx_stream_synchronize(stream))
        need = int(d_need.to_host(np.uint64, 1)[0])
        cap = need if adj_cap is None else adj_cap(need)
        room = max(need, cap) + 64
        d_adj = nat.DeviceBuffer.from_host(np.full(room * 4, pattern, np.uint8))
        nat.cdr3_neighbours_device(m, d_cls, d_off, d_text, len(text), D, d_deg, d_adj_off, d_adj, cap, d_need, d_work, wb, stream, metric=metric)
        nat.check(nat.lib().dcrx_stream_synchronize(stream))
    finally:
        nat.lib().dcrx_stream_destroy(stream)
    assert int(d_need.to_host(np.uint64, 1)[0]) == need
    return d_deg.to_host(np.uint32, m), d_adj_off.to_host(np.uint64, m + 1), d_adj.to_host(np.uint32, room), need, cap


def test_primitive_work_space_and_adjacency_rules():
    strings = clu.families_indel(1500, seed=9, length=13)
    classes = [k % 3 for k in range(1500)]
    want, st = clu.expected_lev_network(classes, strings, [1] * 1500, 2)
    off, text = cnu.node_text(strings)
    with pytest.raises(nat.DcrxError, match="work space is smaller") as e:
        _primitive(classes, strings, 2, work_bytes=nat.cdr3net_work_bytes(1500, len(text), metric=LEV) - 1)
    assert e.value.code == -1
    with pytest.raises(nat.DcrxError, match="work space is smaller"):      # the Hamming size is not enough
        _primitive(classes, strings, 2, work_bytes=nat.cdr3net_work_bytes(1500, len(text)))
    assert nat.cdr3net_work_bytes(1500, len(text), metric="hamming") == nat.cdr3net_work_bytes(1500, len(text))
    assert nat.cdr3net_work_bytes(1500, len(text), metric=LEV) >= nat.cdr3net_work_bytes(1500, len(text)) + 1500 * 4
    filler = 0xA5A5A5A5
    # the exact cap: the CSR of the host entry (and of the contract)
    deg, adj_off, adj, need, cap = _primitive(classes, strings, 2)
    assert need == cap == 2 * st["edges"] == int(adj_off[-1]) and need > 1000
    assert np.array_equal(deg, want["degree"]) and np.array_equal(adj_off, want["adj_off"]) and np.array_equal(adj[:need], want["adj"])
    assert (adj[need:] == filler).all()
    host, _ = nat.cdr3_network(classes, off, text, [1] * 1500, 2, want_edges=True, metric=LEV)
    assert np.array_equal(host["adj"], adj[:need]) and np.array_equal(host["adj_off"], adj_off)
    # half the need: the same need, nothing behind the cap is touched, and what was written in front of it is right
    deg2, adj_off2, adj2, need2, cap2 = _primitive(classes, strings, 2, adj_cap=lambda n: n // 2)
    assert need2 == need and cap2 == need // 2 and np.array_equal(deg2, deg) and np.array_equal(adj_off2, adj_off)
    assert (adj2[cap2:] == filler).all()
    written = adj2[:cap2] != filler
    assert written.any() and np.array_equal(adj2[:cap2][written], want["adj"][:cap2][written])


def test_metric_zero_gives_the_old_entry_arrays():
    strings = cnu.families(1500, seed=9, length=13) + clu.families_indel(500, seed=2, length=13)
    classes = [k % 3 for k in range(2000)]
    for D in (1, 2):
        new = _primitive(classes, strings, D, metric="hamming")
        old = _primitive(classes, strings, D, metric=None)      # dcrx_cdr3_neighbours_device itself
        assert new[3] == old[3] > 500
        for a, b in zip(new[:3], old[:3]):
            assert np.array_equal(a, b)
    off, text = cnu.node_text(strings)
    w = list(range(1, 2001))
    cnu.assert_same(nat.cdr3_network(classes, off, text, w, 2, want_edges=True, metric="hamming"),
                    nat.cdr3_network(classes, off, text, w, 2, want_edges=True))
    cnu.assert_same(nat.cdr3_network(classes, off, text, w, 2, want_edges=True, metric="hamming"), cnu.expected_network(classes, strings, w, 2))


# ---- the stage, end to end ----

def _coding_workdir(tmp_path):
    fx = json.load(open(cu.CODING_FX))
    ts = fx["tagset"]
    t = synth.TagSet(species=ts["species"], tags=ts["tags"], chain=ts["chain"], v_tags=ts["v_tags"], v_jumps=ts["v_jumps"],
                     v_names=ts["v_names"], v_regions=ts["v_regions"], j_tags=ts["j_tags"], j_jumps=ts["j_jumps"],
                     j_names=ts["j_names"], j_regions=ts["j_regions"])
    cu.write_gene_files(tmp_path / "tags", t, fx["genes"])
    (tmp_path / "COD_1.fq").write_text(fx["fastq_r1"])
    (tmp_path / "COD_2.fq").write_text(fx["fastq_r2"])
    return fx, ts


@pytest.mark.parametrize("extra,mode,D", [(["-dz"], "v", 1), ([], "none", 2)], ids=["plain-v-1", "gzip-none-2"])
def test_pipeline_count_dcrs_clonotypes_cdr3_network_levenshtein(extra, mode, D, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    fx, ts = _coding_workdir(tmp_path)
    base = ["pipeline", "-in", "COD_1.fq", "-br", "R2", "-nbc", "--count-dcrs", "--clonotypes", "-tfdir", "tags", "-tg", ts["tags"],
            "-sp", ts["species"], "-c", ts["chain"], "-dc", "-s"] + extra
    opener, gz = (open, "") if "-dz" in extra else (gzip.open, ".gz")
    pipeline.main(base)
    clon = opener(tmp_path / ("dcr_COD_1_beta.clonotypes.tsv" + gz), "rt").read()
    pipeline.main(base + ["--cdr3-network", "--write-cdr3-edges", "--cdr3-metric", "levenshtein", "--cdr3-class", mode, "--cdr3-distance", str(D)])
    assert opener(tmp_path / ("dcr_COD_1_beta.clonotypes.tsv" + gz), "rt").read() == clon
    rows = [ln.split("\t") for ln in clon.splitlines()[1:]]
    v, j, aa, dup = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [int(r[3]) for r in rows]
    result, stats = clu.expected_lev_network(cnu.call_classes(v, j, mode), aa, dup, D)
    assert opener(tmp_path / ("dcr_COD_1_beta.cdr3_clusters.tsv" + gz), "rt").read() == cnu.file_text(v, j, aa, dup, result)
    assert opener(tmp_path / ("dcr_COD_1_beta.cdr3_edges.tsv" + gz), "rt").read() == clu.edges_text(aa, result)
    from decombinator_amd import translate
    assert translate.cdr3_network_stats == stats and stats["nodes_in"] == len(rows) > 300
