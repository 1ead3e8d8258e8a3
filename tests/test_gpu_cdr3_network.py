"""The CDR3 network (`--clonotypes --cdr3-network`) through the HIP path: dcrx_cdr3_network against the contract written in
Python (cnu.expected_network) — degree, the CSR adjacency, cluster_of, the cluster rows and the statistics, exactly — on
degenerate inputs, buckets across tile and block edges, every length and difference position, raw bytes, long component
chains and random families; the primitive's work space and adjacency rules; and the stage end to end."""
import ctypes as C
import gzip
import json
import random

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import pipeline, synth
from tests import cdr3_network_util as cnu
from tests import clonotype_util as cu

pytestmark = pytest.mark.gpu


def _run(classes, strings, D, weights=None, want_edges=True):
    off, text = cnu.node_text(strings)
    w = [1 + (7 * k) % 13 for k in range(len(strings))] if weights is None else weights
    return nat.cdr3_network(classes, off, text, w, D, want_edges=want_edges), w


def _check(classes, strings, D, weights=None):
    """The native result with edges (and the one without) against the contract; returns the expected (result, stats)."""
    got, w = _run(classes, strings, D, weights)
    want = cnu.expected_network(classes, strings, w, D)
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
    assert _check([0, 0], ["CASSF", "CASSY"], D)[1]["edges"] == 1
    assert _check([0, 0], ["CASSF", "CAWWY"], D)[1]["edges"] == 0
    assert _check([0, 1], ["CASSF", "CASSF"], D)[1]["edges"] == 0


def test_every_node_out_of_reach():
    strings = ["", "A" * 33, "", "C" * 40, "A" * 33] * 70
    _, st = _check([0] * len(strings), strings, 1)
    assert st["out_of_reach"] == st["clusters_out"] == st["singletons"] == 350 and st["edges"] == 0


def test_one_bucket_of_identical_strings():
    _, st = _check([0] * 300, ["CASSLGQAYEQYF"] * 300, 1)
    assert st["edges"] == 300 * 299 // 2 and st["clusters_out"] == 1 and st["largest_degree"] == 299


# ---- buckets against tiles and blocks ----

@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_one_bucket_across_tile_boundaries(n):
    """One bucket (class 0, length 12) of n nodes: it ends one before, on and one behind a tile and a block of 256, and in a
    third; the lanes of the last tile run past the end."""
    strings = cnu.families(n, seed=n, length=12)
    _, st = _check([0] * n, strings, 1 + n % 2)
    assert st["edges"] > n // 4 and st["out_of_reach"] == 0


def test_many_small_buckets_in_one_block():
    """600 nodes in buckets of 1 to 7 (one class each, ranks shuffled): a block holds dozens of buckets, buckets straddle the
    blocks' edges, and every bucket is a family around one seed."""
    rnd = random.Random(21)
    nodes, cls = [], 0
    while len(nodes) < 600:
        seed = "".join(rnd.choice(cnu.AMINO) for _ in range(14))
        for _ in range(min(1 + cls % 7, 600 - len(nodes))):
            nodes.append((cls, cnu.mutate(seed, rnd.randrange(0, 3), rnd)))
        cls += 1
    rnd.shuffle(nodes)
    for D in (1, 2):
        _, st = _check([c for c, _ in nodes], [s for _, s in nodes], D)
        assert st["edges"] > 100 and st["clusters_out"] >= cls


def test_a_bucket_that_starts_at_the_last_lane_of_a_block():
    strings = cnu.families(255, seed=5, length=10) + cnu.families(300, seed=6, length=10)
    classes = [0] * 255 + [1] * 300        # class 1 starts at sorted position 255
    _, st = _check(classes, strings, 2)
    assert st["edges"] > 200
    # ... and with a bucket of nodes out of reach in front of it in rank order (they sort behind every bucket)
    _check([0] * 50 + classes, [""] * 25 + ["A" * 33] * 25 + strings, 1)


# ---- decoys: equal packed words in neighbouring buckets, classes that differ in their high bits ----

@pytest.mark.parametrize("D", [1, 2])
def test_a_zero_byte_lengthens_a_string_into_the_next_bucket(D):
    """b"CASSF", b"CASSF\\0" and b"CASSF\\0\\0" (and a pair of 31 and 32 bytes) pack to the same dwords; only the key keeps them
    apart.  The three buckets straddle sorted position 256."""
    classes, strings, at = cnu.zero_byte_run(cnu.families(cnu.ZERO_RUN_FRONT, seed=41, length=6))
    r, st = _check(classes, strings, D)
    assert r["degree"][at:].tolist() == [1, 0, 0, 0, 0, 1] and cnu.no_edge_across(classes, r)


@pytest.mark.parametrize("pair", cnu.CLASS_BIT_PAIRS, ids=["bit31", "bit26", "all-ones"])
def test_classes_that_differ_in_their_high_bits(pair):
    """The same strings under two classes that differ in bit 31, in bit 26 (the key's bit 32) and in bit 0 of 0xFFFFFFFF (with
    nodes out of reach, which sort directly behind that class): the edges are those under classes 0 and 1."""
    classes, strings, plain = cnu.class_bit_nodes(cnu.families(150, seed=43, length=12), pair, n_out=40 if pair[1] == 0xFFFFFFFF else 0)
    w = [1 + (7 * k) % 13 for k in range(len(strings))]
    for D in (1, 2):
        want = _check(classes, strings, D)
        cnu.assert_same(want, cnu.expected_network(plain, strings, w, D))
        assert want[1]["edges"] > 100 and cnu.no_edge_across(classes, want[0])


# ---- lengths and difference positions ----

@pytest.mark.parametrize("D", [1, 2])
def test_lengths_and_difference_positions(D):
    """Lengths 1, 4, 5, 31, 32 and 33 together, each with strings that differ from a base at the first and last byte of the
    first and last dword, alone and in pairs and threes."""
    rnd = random.Random(31)
    strings = []
    for L in (1, 4, 5, 31, 32, 33):
        base = "".join(rnd.choice(cnu.AMINO) for _ in range(L))
        spots = sorted({p for p in (0, 3, 4, L - 4, L - 1) if 0 <= p < L})
        strings.append(base)
        for k in (1, 2, 3):
            for _ in range(6):
                if k <= len(spots):
                    t = list(base)
                    for p in rnd.sample(spots, k):
                        t[p] = rnd.choice([c for c in cnu.AMINO if c != t[p]])
                    strings.append("".join(t))
    rnd.shuffle(strings)
    _, st = _check([0] * len(strings), strings, D)
    assert st["out_of_reach"] == sum(1 for s in strings if len(s) == 33) > 0 and st["edges"] > 20


def test_bytes_are_compared_as_they_are():
    base = [b"CASSLGQAYEQYF", b"CASSLGQAYEQYW", b"casslgqayeqyf", b"CASSLGQAYEQyF", b"CASSL\x80QAYEQYF", b"CASSL\xffQAYEQYF",
            b"CASSLXQAYEQYF", b"CASSL*QAYEQYF", b"CASSL\x00QAYEQYF", b"\xff" * 32, b"\x7f" + b"\xff" * 31, b"\xff" * 31 + b"\x7f"]
    strings = base + base                   # the same strings in two classes
    classes = [0] * len(base) + [1] * len(base)
    for D in (1, 2):
        (r, st) = _check(classes, strings, D)
        assert st["edges"] % 2 == 0 and int(r["degree"][2]) == 0      # lower case is another string
        assert r["adj"].max() < len(strings) and not set(r["adj"][int(r["adj_off"][0]):int(r["adj_off"][1])].tolist()) & set(range(len(base), 2 * len(base)))
    both, _ = _check([0] * len(strings), strings, 1)      # under one class every string meets its twin at distance 0
    assert int(both["degree"][2]) == 1


# ---- component rounds ----

def test_a_shuffled_path_takes_many_rounds():
    strings, rank = cnu.path(200)
    r, st = _check([0] * 200, strings, 1)
    assert st["clusters_out"] == 1 and st["edges"] == 199 and st["largest_degree"] == 2


def test_a_star_adds_onto_one_head():
    r, st = _check([0] * 300, cnu.star(300), 1, weights=[1 << 40] * 300)
    assert st["clusters_out"] == 1 and st["largest_degree"] == 299 and int(r["cluster_weight"][0]) == 300 << 40


def test_two_components_joined_between_the_first_and_the_last_rank():
    c1, c2 = "A" * 24, "A" * 23 + "W"
    l1 = [c1[:t] + "C" + c1[t + 1:] for t in range(20)]
    l2 = [c2[:t] + "D" + c2[t + 1:] for t in range(20)]
    r, st = _check([0] * 42, [c1] + l1 + l2 + [c2], 1)
    assert st["clusters_out"] == 1 and st["edges"] == 41 and int(r["degree"][0]) == int(r["degree"][41]) == 21
    apart = "A" * 22 + "WW"
    _, st = _check([0] * 42, [c1] + l1 + [x[:22] + "WW" for x in l2] + [apart], 1)
    assert st["clusters_out"] == 2


# ---- random families ----

@pytest.fixture(scope="module")
def family_strings():
    return cnu.families(20000, seed=7)


@pytest.mark.parametrize("D,n_classes", [(1, 1), (2, 1), (1, 16), (2, 16)])
def test_random_families_equal_the_brute_force(family_strings, D, n_classes):
    """cnu.families(20000, seed=7): 20-letter seeds, each with a family of 3 to 10 strings mutated in 1 to 3 places.  With 16
    classes a node's class is its first letter's number modulo 16, so that most of a family shares it.  The brute force's
    figures (edges / clusters / singletons / largest cluster / largest degree): class none, D=1: 11 429 / 9 557 / 6 910 / 11 /
    9; D=2: 34 802 / 6 048 / 3 379 / 11 / 10; 16 classes, D=1: 10 839 / 10 092 / 7 460 / 11 / 9; D=2: 31 919 / 6 896 / 4 218 /
    11 / 10 — 1.1 neighbours per node at D=1 and 3.5 at D=2, in half a second (D=1) and five seconds (D=2) of one CPU thread."""
    classes = [0 if n_classes == 1 else cnu.AMINO.index(x[0]) % n_classes for x in family_strings]
    _, st = _check(classes, family_strings, D)
    assert st["edges"] >= 10000 * D and st["largest_cluster"] >= 8      # (no degenerate input passes for a result)


# ---- the primitive ----

def _primitive(classes, strings, D, work_bytes=None, adj_cap=None, pattern=0xA5):
    """dcrx_cdr3_neighbours_device over buffers and a stream of the caller's: (degree, adj_off, the whole adj buffer, need)."""
    m = len(strings)
    off, text = cnu.node_text(strings)
    d_cls = nat.DeviceBuffer.from_host(np.asarray(classes, dtype=np.uint32))
    d_off = nat.DeviceBuffer.from_host(off)
    d_text = nat.DeviceBuffer.from_host(np.frombuffer(text + b"\0", np.uint8))
    d_deg, d_adj_off, d_need = nat.DeviceBuffer(max(16, m * 4)), nat.DeviceBuffer((m + 1) * 8), nat.DeviceBuffer(16)
    wb = nat.cdr3net_work_bytes(m, len(text)) if work_bytes is None else work_bytes
    assert wb > m * 32 or work_bytes is not None
    d_work = nat.DeviceBuffer(max(256, wb))
    stream = C.c_void_p()
    nat.check(nat.lib().dcrx_stream_create(C.byref(stream)))
    try:
        # sized first (no adjacency), then written into one of `adj_cap` entries (default: exactly the need)
        nat.cdr3_neighbours_device(m, d_cls, d_off, d_text, len(text), D, d_deg, d_adj_off, None, 0, d_need, d_work, wb, stream)
        nat.check(nat.lib().dcrx_stream_synchronize(stream))
        need = int(d_need.to_host(np.uint64, 1)[0])
        cap = need if adj_cap is None else adj_cap(need)
        room = max(need, cap) + 64
        d_adj = nat.DeviceBuffer.from_host(np.full(room * 4, pattern, np.uint8))
        nat.cdr3_neighbours_device(m, d_cls, d_off, d_text, len(text), D, d_deg, d_adj_off, d_adj, cap, d_need, d_work, wb, stream)
        nat.check(nat.lib().dcrx_stream_synchronize(stream))
    finally:
        nat.lib().dcrx_stream_destroy(stream)
    assert int(d_need.to_host(np.uint64, 1)[0]) == need
    return d_deg.to_host(np.uint32, m), d_adj_off.to_host(np.uint64, m + 1), d_adj.to_host(np.uint32, room), need, cap


def test_primitive_work_space_and_adjacency_rules():
    strings = cnu.families(1500, seed=9, length=13)
    classes = [k % 3 for k in range(1500)]
    want, st = cnu.expected_network(classes, strings, [1] * 1500, 2)
    off, text = cnu.node_text(strings)
    with pytest.raises(nat.DcrxError, match="work space is smaller") as e:
        _primitive(classes, strings, 2, work_bytes=nat.cdr3net_work_bytes(1500, len(text)) - 1)
    assert e.value.code == -1
    filler = 0xA5A5A5A5
    # the exact cap: the CSR of the host entry (and of the contract)
    deg, adj_off, adj, need, cap = _primitive(classes, strings, 2)
    assert need == cap == 2 * st["edges"] == int(adj_off[-1]) and need > 1000
    assert np.array_equal(deg, want["degree"]) and np.array_equal(adj_off, want["adj_off"]) and np.array_equal(adj[:need], want["adj"])
    assert (adj[need:] == filler).all()
    host, _ = nat.cdr3_network(classes, off, text, [1] * 1500, 2, want_edges=True)
    assert np.array_equal(host["adj"], adj[:need]) and np.array_equal(host["adj_off"], adj_off)
    # half the need: the same need, nothing behind the cap is touched, and what was written in front of it is right
    deg2, adj_off2, adj2, need2, cap2 = _primitive(classes, strings, 2, adj_cap=lambda n: n // 2)
    assert need2 == need and cap2 == need // 2 and np.array_equal(deg2, deg) and np.array_equal(adj_off2, adj_off)
    assert (adj2[cap2:] == filler).all()
    written = adj2[:cap2] != filler
    assert written.any() and np.array_equal(adj2[:cap2][written], want["adj"][:cap2][written])


# ---- the stage, end to end ----

def _coding_workdir(tmp_path):
    """The coding fixture's tag set, gene tables and FASTQ files as files; returns (fixture, tag set)."""
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
def test_pipeline_count_dcrs_clonotypes_cdr3_network(extra, mode, D, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    fx, ts = _coding_workdir(tmp_path)
    base = ["pipeline", "-in", "COD_1.fq", "-br", "R2", "-nbc", "--count-dcrs", "--clonotypes", "-tfdir", "tags", "-tg", ts["tags"],
            "-sp", ts["species"], "-c", ts["chain"], "-dc", "-s"] + extra
    opener, gz = (open, "") if "-dz" in extra else (gzip.open, ".gz")
    pipeline.main(base)
    clon = opener(tmp_path / ("dcr_COD_1_beta.clonotypes.tsv" + gz), "rt").read()
    pipeline.main(base + ["--cdr3-network", "--write-cdr3-edges", "--cdr3-class", mode, "--cdr3-distance", str(D)])
    assert opener(tmp_path / ("dcr_COD_1_beta.clonotypes.tsv" + gz), "rt").read() == clon
    rows = [ln.split("\t") for ln in clon.splitlines()[1:]]
    v, j, aa, dup = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [int(r[3]) for r in rows]
    result, stats = cnu.expected_network(cnu.call_classes(v, j, mode), aa, dup, D)
    assert opener(tmp_path / ("dcr_COD_1_beta.cdr3_clusters.tsv" + gz), "rt").read() == cnu.file_text(v, j, aa, dup, result)
    assert opener(tmp_path / ("dcr_COD_1_beta.cdr3_edges.tsv" + gz), "rt").read() == cnu.edges_text(aa, result)
    from decombinator_amd import translate
    assert translate.cdr3_network_stats == stats and stats["nodes_in"] == len(rows) > 300
