"""The CDR3 network (`--clonotypes --cdr3-network`) without a GPU: the per-node and per-pair code (dcrx_cdr3net_core.h, built
by g++) against Python, the contract's brute force (cnu.expected_network) against hand-made cases whose answers are written
out here, the host-only formatters, and the stage — flags, classes, files, two chains, refusals — with the brute force put in
for _native.cdr3_network."""
import gzip
import json
import os
import random
import subprocess

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import io as dio
from decombinator_amd import pipeline, synth, translate
from tests import cdr3_network_util as cnu
from tests import clonotype_util as cu
from tests import collapse_cluster_util as ccu
from tests import golden_util as gu
from tests import nbc_count_util as nu
from tests import parity_util as pu


# ---- the core on the host against Python ----

def _py_pack(s: bytes):
    w = [0] * 8
    if 1 <= len(s) <= 32:
        for p, c in enumerate(s):
            w[p // 4] |= c << (8 * (p % 4))
    return w


def test_core_reach_keys_and_packing():
    H = cnu.host_lib()
    assert H.cdr3net_host_words() == 8 and H.cdr3net_host_max_len() == 32 == nat.CDR3NET_MAX_LEN
    oor = H.cdr3net_host_key_out_of_reach()
    assert oor < (1 << H.cdr3net_host_key_bits())
    assert [H.cdr3net_host_in_reach(n) for n in (0, 1, 32, 33, 1 << 40)] == [0, 1, 1, 0, 0]
    rnd = random.Random(3)
    keys = {}
    for cls in [0, 1, 59, 0xFFFFFFFF] + [rnd.randrange(1 << 32) for _ in range(50)]:
        for n in (0, 1, 2, 31, 32, 33, 200):
            k = H.cdr3net_host_key(cls, n)
            if 1 <= n <= 32:
                assert k < oor and keys.setdefault(k, (cls, n)) == (cls, n)      # one key per (class, length), before the rest
            else:
                assert k == oor
    # the keys order by class first, then by length: a bucket is a run of the sorted keys
    assert H.cdr3net_host_key(3, 32) < H.cdr3net_host_key(4, 1) and H.cdr3net_host_key(3, 7) < H.cdr3net_host_key(3, 8)
    for n in (0, 1, 3, 4, 5, 16, 17, 31, 32, 33, 40):
        s = bytes(rnd.randrange(256) for _ in range(n))
        assert cnu.host_pack(s).tolist() == _py_pack(s), n


@pytest.mark.parametrize("D", [1, 2])
def test_core_hamming_gives_up_past_the_limit(D):
    H = cnu.host_lib()
    rnd = random.Random(10 + D)

    def dist(a, b):
        pa, pb = cnu.host_pack(a), cnu.host_pack(b)
        return H.cdr3net_host_distance(pa.ctypes.data, pb.ctypes.data, D)
    # one difference at the first and last byte of the first and last dword, and in the middle
    base = bytes(rnd.choice(cnu.AMINO.encode()) for _ in range(32))
    for p in (0, 3, 4, 28, 31):
        other = base[:p] + bytes([base[p] ^ 0x20]) + base[p + 1:]
        assert dist(base, other) == 1 and dist(other, base) == 1, p
        assert dist(base[:p + 1], other[:p + 1]) == 1
    assert dist(base, base) == 0
    # exactly D, and D + 1, at every pair of those positions and at random ones
    for _ in range(300):
        n = rnd.randrange(1, 33)
        a = bytes(rnd.randrange(256) for _ in range(n))
        for k in (D, D + 1, rnd.randrange(0, n + 1)):
            if k > n:
                continue
            b = bytearray(a)
            for p in rnd.sample(range(n), k):
                b[p] = (b[p] + 1 + rnd.randrange(255)) % 256
            want = sum(x != y for x, y in zip(a, b))
            assert want == k
            got = dist(a, bytes(b))
            assert got == want if want <= D else got > D, (a, b, got)
    # a byte's value does not matter, only whether it is the same: case, 'X', '*', bytes >= 0x80
    assert dist(b"CASSL", b"cASSL") == 1 and dist(b"CAXSL", b"CA*SL") == 1 and dist(b"CA\x80SL", b"CA\xffSL") == 1
    assert dist(b"CA\x00SL", b"CA\x00SL") == 0 and dist(b"\xff" * 32, b"\x7f" * 32) > D


def test_sanitizer_run_of_the_host_walk():
    """The network's two plain walks (Within with Hamming and with Levenshtein) in a stand-alone program (its own main) under
    AddressSanitizer and UBSan: host code, on the CPU."""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_cdr3net")
    got = subprocess.run(["make", "-s", "-C", here, "asan"], capture_output=True, text=True)
    assert got.returncode == 0, got.stdout[-2000:] + got.stderr[-2000:]
    assert got.stdout.splitlines()[-1] == "ok" and "rows differ" in got.stdout and "classes over block edges" in got.stdout


# ---- the brute force against answers written out here ----

def _net(classes, strings, D, weights=None):
    w = list(range(1, len(strings) + 1)) if weights is None else weights
    return cnu.expected_network(classes, strings, w, D)


def test_two_classes_keep_the_same_string_apart():
    r, st = _net([0, 1], ["CASSF", "CASSF"], 1)
    assert r["degree"].tolist() == [0, 0] and r["cluster_of"].tolist() == [0, 1] and r["cluster_head"].tolist() == [0, 1]
    assert r["adj_off"].tolist() == [0, 0, 0] and len(r["adj"]) == 0 and r["cluster_weight"].tolist() == [1, 2]
    assert st == {"nodes_in": 2, "out_of_reach": 0, "edges": 0, "clusters_out": 2, "singletons": 2, "largest_cluster": 1, "largest_degree": 0}


def test_distance_zero_is_an_edge_under_class_none():
    r, st = _net([0, 0, 0], ["CASSF", "CASSY", "CASSF"], 1, [5, 3, 2])
    assert r["degree"].tolist() == [2, 2, 2] and r["adj"].tolist() == [1, 2, 0, 2, 0, 1] and r["adj_off"].tolist() == [0, 2, 4, 6]
    assert r["cluster_of"].tolist() == [0, 0, 0] and r["cluster_size"].tolist() == [3] and r["cluster_weight"].tolist() == [10]
    assert st["edges"] == 3 and st["singletons"] == 0
    # lengths apart, and strings out of reach (empty, 33 bytes): clusters of their own, counted
    r, st = _net([0] * 5, ["CASSF", "CASS", "", "A" * 33, "A" * 33], 2)
    assert r["degree"].tolist() == [0] * 5 and r["cluster_of"].tolist() == [0, 1, 2, 3, 4] and st["out_of_reach"] == 3 and st["singletons"] == 5


def test_a_path_is_one_cluster():
    strings, rank = cnu.path(6)
    assert sorted(rank) == list(range(6)) and rank != list(range(6))
    r, st = _net([0] * 6, strings, 1)
    assert [int(r["degree"][rank[t]]) for t in range(6)] == [1, 2, 2, 2, 2, 1]
    for t in range(5):
        a, b = rank[t], rank[t + 1]
        assert b in r["adj"][int(r["adj_off"][a]):int(r["adj_off"][a + 1])].tolist()
    assert r["cluster_of"].tolist() == [0] * 6 and r["cluster_head"].tolist() == [0] and r["cluster_size"].tolist() == [6]
    assert r["cluster_weight"].tolist() == [21] and st["edges"] == 5 and st["largest_degree"] == 2
    # at distance 2 every string also reaches the next but one
    r2, st2 = _net([0] * 6, strings, 2)
    assert [int(r2["degree"][rank[t]]) for t in range(6)] == [2, 3, 4, 4, 3, 2] and st2["edges"] == 9
    # the generator's claim, on the longest path: consecutive at 1, all others at >= 2
    long, rk = cnu.path(200)
    by_t = [long[rk[t]] for t in range(200)]
    for a in range(200):
        for b in range(a + 1, 200):
            d = sum(x != y for x, y in zip(by_t[a], by_t[b]))
            assert d == 1 if b == a + 1 else d >= 2


def test_a_star():
    strings = cnu.star(5)
    r, st = _net([0] * 5, strings, 1)
    assert r["degree"].tolist() == [1, 1, 1, 1, 4] and r["adj"].tolist() == [4, 4, 4, 4, 0, 1, 2, 3]
    assert r["cluster_head"].tolist() == [0] and r["cluster_size"].tolist() == [5] and r["cluster_weight"].tolist() == [15]
    assert st["edges"] == 4 and st["largest_degree"] == 4 and st["largest_cluster"] == 5
    r2, st2 = _net([0] * 5, strings, 2)       # the leaves are two apart
    assert r2["degree"].tolist() == [4] * 5 and st2["edges"] == 10


def test_two_stars_joined_by_one_edge_between_the_first_and_the_last_rank():
    c1, c2 = "AAAAAAAAAA", "AAAAAAAAAC"
    l1 = ["CAAAAAAAAA", "ACAAAAAAAA", "AACAAAAAAA"]
    l2 = ["AAADAAAAAC", "AAAADAAAAC", "AAAAADAAAC"]
    r, st = _net([0] * 8, [c1] + l1 + l2 + [c2], 1)
    assert r["degree"].tolist() == [4, 1, 1, 1, 1, 1, 1, 4] and r["adj"][:4].tolist() == [1, 2, 3, 7] and r["adj"][-4:].tolist() == [0, 4, 5, 6]
    assert r["cluster_of"].tolist() == [0] * 8 and r["cluster_size"].tolist() == [8] and st["edges"] == 7
    # without the joining edge (the second centre two away from the first): two clusters, the second headed by its first leaf
    c3, l3 = "AAAAAAAACC", [x[:8] + "CC" for x in l2]
    r, st = _net([0] * 8, [c1] + l1 + l3 + [c3], 1)
    assert r["cluster_of"].tolist() == [0, 0, 0, 0, 1, 1, 1, 1] and r["cluster_head"].tolist() == [0, 4] and st["edges"] == 6
    assert r["cluster_weight"].tolist() == [1 + 2 + 3 + 4, 5 + 6 + 7 + 8]


def test_the_generators_make_neighbours():
    s = cnu.families(2000, seed=1)
    r, st = cnu.expected_network([0] * len(s), s, [1] * len(s), 1)
    assert len(s) == 2000 and 500 < st["edges"] < 10000 and st["largest_cluster"] >= 3
    full = cnu.star(300)
    assert len(set(full)) == 300 and full[-1] == "A" * 20


# ---- the host pieces of the native side ----

def test_formatters_and_the_empty_network_need_no_device():
    strings = ["CASSF", "CASSY", "CASSF", "", "CAW"]
    classes, w = [0, 0, 0, 0, 1], [9, 4, 2, 1, 1]
    result, stats = cnu.expected_network(classes, strings, w, 1)
    off, text = cnu.node_text(strings)
    v_calls, j_calls = ["TRBV1", "TRBV2"], ["TRBJ1"]
    v_idx, j_idx = [0, 0, 0, 0, 1], [0] * 5
    got = nat.format_cdr3_clusters(v_idx, j_idx, v_calls, j_calls, off, text, w, result).decode()
    assert got == cnu.file_text([v_calls[k] for k in v_idx], ["TRBJ1"] * 5, strings, w, result)
    assert got.splitlines()[0].split("\t") == nat.CDR3_CLUSTER_COLUMNS
    assert got.splitlines()[1] == "0\tTRBV1\tTRBJ1\tCASSF\t9\t0\t3\t15\t2" and got.splitlines()[4] == "3\tTRBV1\tTRBJ1\t\t1\t1\t1\t1\t0"
    edges = nat.format_cdr3_edges(off, text, result).decode()
    assert edges == cnu.edges_text(strings, result) == "a\tb\tdistance\n0\t1\t1\n0\t2\t0\n1\t2\t1\n"
    with pytest.raises(nat.DcrxError, match="outside its table"):
        nat.format_cdr3_clusters([2] * 5, j_idx, v_calls, j_calls, off, text, w, result)
    # no node: nothing is launched
    e_off, e_text = cnu.node_text([])
    got = nat.cdr3_network([], e_off, e_text, [], 1, want_edges=True)
    cnu.assert_same(got, cnu.expected_network([], [], [], 1))
    assert nat.format_cdr3_clusters([], [], v_calls, j_calls, e_off, e_text, [], got[0]).decode() == "\t".join(nat.CDR3_CLUSTER_COLUMNS) + "\n"
    assert nat.format_cdr3_edges(e_off, e_text, got[0]).decode() == "a\tb\tdistance\n"
    # refused before the device is touched
    assert nat.cdr3net_work_bytes(1 << 30, 0) == 0
    for bad in (0, 3):
        with pytest.raises(nat.DcrxError, match="1 or 2") as e:
            nat.cdr3_network(classes, off, text, w, bad)
        assert e.value.code == -1
    back = off.copy()
    back[2] = 0
    with pytest.raises(nat.DcrxError, match="backwards") as e:
        nat.cdr3_network(classes, back, text, w, 1)
    assert e.value.code == -1


def test_the_abi_version_stays():
    assert nat.ABI_VERSION == 5 == nat.lib().dcrx_abi_version()
    assert [f[0] for f in nat.Cdr3NetworkStatsC._fields_] == list(nat.CDR3_NETWORK_STATS)


# ---- the stage, with the brute forces as _native.clonotypes and _native.cdr3_network ----

@pytest.fixture()
def coding(tmp_path, monkeypatch):
    """The coding fixture as files in a working directory, the oracle as the device, the brute forces as the native functions."""
    monkeypatch.chdir(tmp_path)
    fx = json.load(open(cu.CODING_FX))
    ts = fx["tagset"]
    t = synth.TagSet(species=ts["species"], tags=ts["tags"], chain=ts["chain"], v_tags=ts["v_tags"], v_jumps=ts["v_jumps"],
                     v_names=ts["v_names"], v_regions=ts["v_regions"], j_tags=ts["j_tags"], j_jumps=ts["j_jumps"],
                     j_names=ts["j_names"], j_regions=ts["j_regions"])
    cu.write_gene_files(tmp_path / "tags", t, fx["genes"])
    (tmp_path / "COD_1.fq").write_text(fx["fastq_r1"])
    (tmp_path / "COD_2.fq").write_text(fx["fastq_r2"])
    G = translate.GeneInfo(**fx["genes"])
    calls = []
    monkeypatch.setattr(nat, "clonotypes", cu.brute_force_native(G))
    monkeypatch.setattr(nat, "cdr3_network", cnu.brute_force_native(calls))
    ot = gu.oracle_tables(ts)
    monkeypatch.setattr(nat, "decombine", lambda tables, batch, orientation="reverse", allow_ns=False, lenthreshold=130, flags=0:
                        pu.oracle_records(ot, nat.unpack_reads(batch), orientation, allow_ns, lenthreshold))
    monkeypatch.setattr(nat, "umi_neighbours", ccu.brute_neighbours)
    nu.OracleCountDevice(monkeypatch)
    common = ["-tfdir", "tags", "-tg", ts["tags"], "-sp", ts["species"], "-c", ts["chain"]]
    return fx, G, calls, common


def _clonotype_columns(text: str):
    """(v_calls, j_calls, junction_aa, duplicate_count) of a `.clonotypes.tsv`'s text."""
    rows = [ln.split("\t") for ln in text.splitlines()[1:]]
    return [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [int(r[3]) for r in rows]


def _want(clonotypes_text: str, mode: str, D: int):
    """(clusters text, edges text, statistics) for the clonotype table a run wrote."""
    v, j, aa, dup = _clonotype_columns(clonotypes_text)
    result, stats = cnu.expected_network(cnu.call_classes(v, j, mode), aa, dup, D)
    return cnu.file_text(v, j, aa, dup, result), cnu.edges_text(aa, result), stats


def test_translate_writes_the_clusters_plain_and_gzipped_and_changes_nothing_else(coding, tmp_path):
    fx, G, calls, common = coding
    pipeline.main(["pipeline", "-in", "COD_1.fq", "-br", "R2", "-nbc", "--count-dcrs", "--clonotypes", "-dc", "-s", "-dz"] + common)
    before = {n: (tmp_path / n).read_bytes() for n in ("dcr_COD_1_beta.clonotypes.tsv", "dcr_COD_1_beta.tsv", "dcr_COD_1_beta.nbc")}
    assert calls == [] and not [x for x in os.listdir(tmp_path) if "cdr3" in x]
    os.mkdir(tmp_path / "plain")
    tr = ["translate", "-in", "dcr_COD_1_beta.nbc", "-nbc", "--count-dcrs", "--clonotypes"] + common
    pipeline.main(tr + ["-dz", "-op", "plain" + os.sep])
    without = {n: (tmp_path / "plain" / n).read_bytes() for n in ("dcr_COD_1_beta.clonotypes.tsv", "dcr_COD_1_beta.tsv")}
    os.mkdir(tmp_path / "net")
    pipeline.main(tr + ["--cdr3-network", "-dz", "-op", "net" + os.sep])
    for n, text in without.items():                        # byte for byte the same with and without the flag
        assert (tmp_path / "net" / n).read_bytes() == text == before[n]
    want, _, stats = _want(without["dcr_COD_1_beta.clonotypes.tsv"].decode(), "v", 1)
    name = tmp_path / "net" / "dcr_COD_1_beta.cdr3_clusters.tsv"
    assert name.read_text() == want and len(want.splitlines()) > 300
    assert oct(os.stat(name).st_mode & 0o777) == "0o666" and not (tmp_path / "net" / "dcr_COD_1_beta.cdr3_edges.tsv").exists()
    assert translate.cdr3_network_stats == stats and stats["nodes_in"] == len(want.splitlines()) - 1
    assert len(calls) == 1 and calls[0][2:] == (1, False)
    # gzipped by default, beside the .tsv.gz
    pipeline.main(tr + ["--cdr3-network"])
    assert gzip.open(tmp_path / "dcr_COD_1_beta.cdr3_clusters.tsv.gz", "rt").read() == want
    assert (tmp_path / "dcr_COD_1_beta.tsv.gz").exists()
    # dontsave: the statistics, no file
    os.mkdir(tmp_path / "none")
    pipeline.main(["pipeline", "-in", "COD_1.fq", "-br", "R2", "-nbc", "--count-dcrs", "--clonotypes", "--cdr3-network", "-dc", "-s", "-ds",
                   "-op", "none" + os.sep] + common)
    assert not [x for x in os.listdir(tmp_path / "none") if "cdr3" in x] and translate.cdr3_network_stats == stats and len(calls) == 3


@pytest.mark.parametrize("mode,D", [("none", 2), ("v", 1), ("vj", 2)])
def test_pipeline_writes_clusters_and_edges_for_every_class(coding, tmp_path, mode, D):
    fx, G, calls, common = coding
    pipeline.main(["pipeline", "-in", "COD_1.fq", "-br", "R2", "-nbc", "--count-dcrs", "--clonotypes", "--cdr3-network", "--write-cdr3-edges",
                   "--cdr3-class", mode, "--cdr3-distance", str(D), "-dc", "-s", "-dz"] + common)
    clon = (tmp_path / "dcr_COD_1_beta.clonotypes.tsv").read_text()
    want, want_edges, stats = _want(clon, mode, D)
    assert (tmp_path / "dcr_COD_1_beta.cdr3_clusters.tsv").read_text() == want
    assert (tmp_path / "dcr_COD_1_beta.cdr3_edges.tsv").read_text() == want_edges
    assert translate.chain_cdr3_network_stats["b"] == translate.cdr3_network_stats == stats
    v, j, aa, _ = _clonotype_columns(clon)
    assert len(calls) == 1 and calls[0][2:] == (D, True) and [s.decode() for s in calls[0][1]] == aa
    assert cnu.same_partition(calls[0][0], cnu.call_classes(v, j, mode))
    if mode == "none":
        assert stats["edges"] > 0 and len(want_edges.splitlines()) == stats["edges"] + 1      # (the fixture has neighbours to find)


def test_classes_follow_the_call_groups_not_the_alleles():
    """Four hand-made clonotypes over cu.coding_genes (V genes 0 and 1 are two alleles of TRBV1, J genes 0 and 1 of TRBJ1):
    under v the alleles share a class, under vj the J call separates, under none nothing does."""
    G = cu.coding_genes(3)
    genes = translate._clono_genes(G)
    aa = ["CASSLGF", "CASSLGW", "CASSLGF", "CASSLGY"]
    off = [0]
    for s in aa:
        off += [off[-1] + len(s), off[-1] + len(s) + 3]       # junction_aa, then a junction of three bytes
    table = {"rep": np.array([0, 1, 2, 3], np.uint32), "duplicate_count": np.array([9, 5, 3, 1], np.uint64),
             "junc_off": np.array(off, np.uint64), "junc_text": "".join(s + "NNN" for s in aa).encode()}
    counted = {"v": np.array([0, 1, 2, -len(G.v_names)], np.int32), "j": np.array([0, 1, 0, 2], np.int32)}
    T = translate.ClonotypeTable(genes, table, counted, {}, None)
    nodes = translate.cdr3_nodes(T, "v")
    assert cnu.node_strings(nodes["aa_off"], nodes["aa_text"]) == [s.encode() for s in aa] and nodes["weights"].tolist() == [9, 5, 3, 1]
    assert nodes["v"].tolist() == [0, 1, 2, 0] and nodes["j"].tolist() == [0, 1, 0, 2]       # (a negative gene counts from the end)
    v_calls, j_calls = [genes.v_calls[k] for k in nodes["v"]], [genes.j_calls[k] for k in nodes["j"]]
    assert v_calls == ["TRBV1", "TRBV1", "TRBV2", "TRBV1"] and j_calls == ["TRBJ1", "TRBJ1", "TRBJ1", "TRBJ2"]
    want = {"none": [0, 0, 0, 0], "v": [0, 0, 1, 0], "vj": [0, 0, 1, 2]}
    for mode, classes in want.items():
        got = translate.cdr3_nodes(T, mode)["classes"].tolist()
        assert cnu.same_partition(got, classes) and cnu.same_partition(got, cnu.call_classes(v_calls, j_calls, mode)), mode
    with pytest.raises(ValueError, match="none, v, vj"):
        translate.cdr3_nodes(T, "j")


def test_two_chains_write_their_own_files(tmp_path, monkeypatch):
    """`pipeline -c a,b ... --cdr3-network --write-cdr3-edges`: each chain's files equal its single-chain run's (the gene import
    is fed a seeded coding gene set per chain, as tests/test_clonotypes.py does)."""
    monkeypatch.chdir(tmp_path)
    nu.OracleCountDevice(monkeypatch)
    ta, tb = synth.config3_tagsets()
    sets = {"a": ta, "b": tb}
    infos = {c: cu.coding_genes(40 + k, len(ts.v_regions), len(ts.j_regions)) for k, (c, ts) in enumerate(sets.items())}
    monkeypatch.setattr(translate, "import_gene_information", lambda inputargs: infos[inputargs["chain"]])
    monkeypatch.setattr(nat, "clonotypes", lambda genes, counted: cu.brute_force_native(translate._genes)(genes, counted))
    monkeypatch.setattr(nat, "cdr3_network", cnu.brute_force_native())
    reads = nu.clonal_reads(ta, 300, seed=31) + nu.clonal_reads(tb, 300, seed=32)
    ta.write(str(tmp_path / "tags"))
    tb.write(str(tmp_path / "tags"))
    nu.write_fastq(tmp_path / "NBC_1.fq", reads)
    base = ["pipeline", "-in", "NBC_1.fq", "-br", "R2", "-nbc", "--count-dcrs", "--clonotypes", "--cdr3-network", "--write-cdr3-edges",
            "--cdr3-class", "none", "--cdr3-distance", "2", "-tfdir", "tags", "-tg", ta.tags, "-sp", ta.species, "-dc", "-s", "-dz"]
    names = [f"dcr_NBC_1_{n}.{kind}.tsv" for n in ("alpha", "beta") for kind in ("cdr3_clusters", "cdr3_edges", "clonotypes")]
    pipeline.main(base + ["-c", "a,b"])
    both = {n: (tmp_path / n).read_text() for n in names}
    stats = {c: dict(translate.chain_cdr3_network_stats[c]) for c in "ab"}
    for c, chain in (("a", "alpha"), ("b", "beta")):
        for n in names:
            os.remove(tmp_path / n) if chain in n else None
        pipeline.main(base + ["-c", c])
        for n in names:
            if chain in n:
                assert (tmp_path / n).read_text() == both[n], n
        assert translate.cdr3_network_stats == stats[c] and stats[c]["nodes_in"] > 3
        want, want_edges, _ = _want(both[f"dcr_NBC_1_{chain}.clonotypes.tsv"], "none", 2)
        assert both[f"dcr_NBC_1_{chain}.cdr3_clusters.tsv"] == want and both[f"dcr_NBC_1_{chain}.cdr3_edges.tsv"] == want_edges
    assert both[names[0]] != both[names[3]]


def test_refusals_before_anything_is_read(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(nat, "FastqReader", lambda *a, **k: pytest.fail("a reader was opened"))
    monkeypatch.setattr(translate, "import_gene_information", lambda *a, **k: pytest.fail("gene files were read"))
    monkeypatch.setattr(nat, "clonotypes", lambda *a, **k: pytest.fail("the device was called"))
    monkeypatch.setattr(nat, "cdr3_network", lambda *a, **k: pytest.fail("the device was called"))
    import builtins
    real_open = builtins.open
    monkeypatch.setattr(gzip, "open", lambda *a, **k: pytest.fail("a file was opened"))
    pl = ["pipeline", "-in", "X_1.fq", "-br", "R2", "-c", "b", "-tfdir", "tags", "-nbc", "--count-dcrs"]
    tr = ["translate", "-in", "dcr_X_1_beta.nbc.gz", "-c", "b", "-nbc", "--count-dcrs"]
    for argv in (pl + ["--cdr3-network"],                                            # no clonotype table
                 tr + ["--cdr3-network"],
                 pl + ["--clonotypes", "--cdr3-distance", "1"],                      # the other three without --cdr3-network
                 pl + ["--clonotypes", "--cdr3-class", "v"],
                 tr + ["--clonotypes", "--write-cdr3-edges"],
                 pl + ["--clonotypes", "--cdr3-network", "--cdr3-distance", "0"],   # a distance other than 1 or 2
                 tr + ["--clonotypes", "--cdr3-network", "--cdr3-distance", "3"],
                 pl + ["--clonotypes", "--cdr3-network", "--cdr3-class", "j"]):
        with pytest.raises(SystemExit) as e:
            pipeline.main(argv)
        assert e.value.code == 2, argv
    assert builtins.open is real_open and os.listdir(tmp_path) == []
    args = dio.create_args_dict(infile="X_1.fq", chain="b", bc_read="R2", tagfastadir="tags", outpath="", command="pipeline", nobarcoding=True,
                                count_dcrs=True, clonotypes=True, cdr3_network=True)
    assert (args["cdr3_distance"], args["cdr3_class"], args["write_cdr3_edges"]) == (1, "v", False)
    assert pipeline.cdr3_network_refusal(args) is None
    assert "needs --clonotypes" in pipeline.cdr3_network_refusal(dict(args, clonotypes=False))
    assert "1 or 2" in pipeline.cdr3_network_refusal(dict(args, cdr3_distance=3))
    assert "--write-cdr3-edges belongs to --cdr3-network" in pipeline.cdr3_network_refusal(dict(args, cdr3_network=False, write_cdr3_edges=True))
    with pytest.raises(ValueError, match="1 or 2"):
        pipeline.run(dict(args, cdr3_distance=3))
    with pytest.raises(ValueError, match="needs --clonotypes"):
        pipeline.run(dict(args, clonotypes=False))
    d = dio.create_args_dict(infile="x", chain="b", bc_read="R2")
    assert d["cdr3_network"] is False and pipeline.cdr3_network_refusal(d) is None
    c = dio.cli_args(["translate", "-in", "x.freq"])
    assert c["cdr3_network"] is False and c["cdr3_distance"] == 1 and c["cdr3_class"] == "v" and c["cdr3_options_given"] == []
