"""The CDR3 network's Levenshtein metric (`--cdr3-network --cdr3-metric levenshtein`) without a GPU: the pair test lev_within
(dcrx_cdr3net_core.h, built by g++) against a plain DP, the contract's brute force against answers written out here, and the
stage — the flag, files, two chains, refusals — with the brute force put in for _native.cdr3_network."""
import gzip
import itertools
import json
import os
import random

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import io as dio
from decombinator_amd import pipeline, synth, translate
from tests import cdr3_lev_util as clu
from tests import cdr3_network_util as cnu
from tests import clonotype_util as cu
from tests import collapse_cluster_util as ccu
from tests import golden_util as gu
from tests import nbc_count_util as nu
from tests import parity_util as pu


def _assert_exact(pairs, D):
    got = clu.host_lev_within_many(pairs, D)
    for (a, b), g in zip(pairs, got.tolist()):
        want = clu.lev(a, b)
        assert (g == want) if want <= D else (g > D), (a, b, D, g, want)


# ---- lev_within on the host against the DP ----

@pytest.mark.parametrize("D", [1, 2])
def test_every_pair_of_short_strings_over_two_letters(D):
    strings = [bytes(t) for n in range(7) for t in itertools.product(b"AB", repeat=n)]
    pairs = [(a, b) for a in strings for b in strings]
    assert len(pairs) == 127 * 127
    _assert_exact(pairs, D)


@pytest.mark.parametrize("D", [1, 2])
def test_random_pairs_up_to_three_edits_apart(D):
    rnd = random.Random(40 + D)
    pairs = []
    for _ in range(100000):
        a = "".join(rnd.choice(cnu.AMINO[:6]) for _ in range(rnd.randrange(1, 33)))      # (few letters: shifted matches abound)
        pairs.append((a.encode(), clu.edit(a, rnd.randrange(0, 4), rnd).encode()))
    _assert_exact(pairs, D)
    near = sum(1 for a, b in pairs[:2000] if clu.lev(a, b) <= D)
    assert 500 < near < 1900      # (both answers are well represented)


def _edits_at(base: bytes, p: int):
    """base with byte p substituted, deleted, and a byte inserted in front of it."""
    other = bytes([base[p] ^ 0x15])
    out = [base[:p] + other + base[p + 1:], base[:p] + base[p + 1:]]
    if len(base) < 32:
        out.append(base[:p] + other + base[p:])
    return out


@pytest.mark.parametrize("D", [1, 2])
def test_edits_at_the_dword_edges(D):
    rnd = random.Random(7)
    pairs = []
    for L in (1, 2, 4, 5, 8, 9, 12, 16, 17, 31, 32):
        base = bytes(rnd.choice(cnu.AMINO.encode()) for _ in range(L))
        spots = sorted({p for p in (0, 3, 4, 7, 8, L - 4, L - 1) if 0 <= p < L})
        ones = [x for p in spots for x in _edits_at(base, p)]
        twos = [y for x in ones for p in spots if p < len(x) for y in _edits_at(x, p) if 1 <= len(y) <= 32]
        for x in ones + twos:
            pairs += [(base, x), (x, base)]
        if L < 32:
            pairs += [(base, base + b"W"), (base + b"W", base), (b"W" + base, base)]
    assert len(pairs) > 2000
    _assert_exact(pairs, D)
    # the lengths at the reach's end
    a = bytes(range(65, 97))
    for D2, want in ((1, 1), (2, 1)):
        assert clu.host_lev_within(a, a[:31], D2) == want and clu.host_lev_within(a[1:], a, D2) == want
    assert clu.host_lev_within(a, a, D) == 0 and clu.host_lev_within(a, a[:16] + b"!" + a[17:], D) == 1
    assert clu.lev(a, a[1:] + b"!") == 2 and (clu.host_lev_within(a, a[1:] + b"!", D) == 2 if D == 2 else clu.host_lev_within(a, a[1:] + b"!", D) > 1)


@pytest.mark.parametrize("D", [1, 2])
def test_runs_of_one_letter_and_raw_bytes(D):
    runs = [b"A" * k for k in range(0, 33)]
    pairs = [(a, b) for a in runs for b in runs]
    _assert_exact(pairs, D)
    for k in range(0, 33):
        for j in range(max(0, k - 3), min(32, k + 3) + 1):
            got = clu.host_lev_within(b"\x00" * k, b"\x00" * j, D)
            assert got == abs(k - j) if abs(k - j) <= D else got > D, (k, j)
    assert clu.host_lev_within(b"CASS\x00", b"CASS", D) == 1 and clu.host_lev_within(b"CASS", b"CASS\x00", D) == 1
    assert clu.host_lev_within(b"\x00CASS", b"CASS", D) == 1 and clu.host_lev_within(b"CASS\x00\x00", b"CASS", D) == min(2, D + 1)
    raw = [b"CASSLGQAYEQYF", b"CASSL\x00QAYEQYF", b"CASSL\x7fQAYEQYF", b"CASSL\x80QAYEQYF", b"CASSL\xffQAYEQYF", b"CASSLgQAYEQYF",
           b"CASSL\x27QAYEQYF", b"CASSLQAYEQYF", b"CASSLG\x00QAYEQYF", b"\xff" * 32, b"\x7f" + b"\xff" * 31, b"\xff" * 31, b"\x00" * 32,
           b"\x00" * 31 + b"\x80", b"A!a\x01\x21\x41\x61\x81", b"A!a\x01\x21\x41\x61", b"!a\x01\x21\x41\x61\x81"]      # (bytes equal modulo 32)
    _assert_exact([(a, b) for a in raw for b in raw], D)


def test_presence_masks_never_reject_a_pair_in_reach():
    H = clu.host_lib()
    assert clu.host_presence(b"") == 0 and clu.host_presence(b"A") == 1 << 1 and clu.host_presence(b"\x00") == 1
    assert clu.host_presence(b"A!a\x01\x81") == 1 << 1 and clu.host_presence(bytes(range(32))) == 0xFFFFFFFF
    assert clu.host_presence(b"ABC" + b"\x00" * 0) == 0b1110      # (padding is not a letter)
    rnd = random.Random(5)
    for _ in range(20000):
        a = bytes(rnd.randrange(256) for _ in range(rnd.randrange(1, 33))).decode("latin-1")
        t = list(a)
        k = rnd.randrange(0, 3)
        for _ in range(k):      # k edits over all 256 byte values
            kind = rnd.randrange(3)
            if kind == 0 or (kind == 1 and len(t) >= 32) or (kind == 2 and len(t) <= 1):
                t[rnd.randrange(len(t))] = chr(rnd.randrange(256))
            elif kind == 1:
                t.insert(rnd.randrange(len(t) + 1), chr(rnd.randrange(256)))
            else:
                del t[rnd.randrange(len(t))]
        pa, pb = clu.host_presence(a.encode("latin-1")), clu.host_presence("".join(t).encode("latin-1"))
        for D in (1, 2):
            if k <= D:
                assert H.cdr3lev_host_presence_allows(pa, pb, D) == 1
    # the class-only bucket: the key's class and length halves
    for cls, n in ((0, 1), (7, 32), (0xFFFFFFFF, 13)):
        key = cnu.host_lib().cdr3net_host_key(cls, n)
        assert H.cdr3lev_host_key_class(key) == cls and H.cdr3lev_host_key_length(key) == n
    assert H.cdr3lev_host_key_class(cnu.host_lib().cdr3net_host_key_out_of_reach()) == 1 << 32


# ---- the brute force against answers written out here ----

def test_the_contract_on_hand_made_cases():
    r, st = clu.expected_lev_network([0, 0, 0, 1, 0, 0], ["CASSF", "CASSFF", "CASSFFF", "CASSF", "", "A" * 33], [1, 2, 3, 4, 5, 6], 1)
    assert r["degree"].tolist() == [1, 2, 1, 0, 0, 0] and r["adj"].tolist() == [1, 0, 2, 1] and r["adj_off"].tolist() == [0, 1, 3, 4, 4, 4, 4]
    assert r["cluster_of"].tolist() == [0, 0, 0, 1, 2, 3] and r["cluster_weight"].tolist() == [6, 4, 5, 6]
    assert st == {"nodes_in": 6, "out_of_reach": 2, "edges": 2, "clusters_out": 4, "singletons": 3, "largest_cluster": 3, "largest_degree": 2}
    off, text = cnu.node_text(["CASSF", "CASSFF", "CASSFFF", "CASSF", "", "A" * 33])
    assert nat.format_cdr3_edges(off, text, r, metric="levenshtein").decode() == "a\tb\tdistance\n0\t1\t1\n1\t2\t1\n"
    r2, st2 = clu.expected_lev_network([0, 0, 0, 1, 0, 0], ["CASSF", "CASSFF", "CASSFFF", "CASSF", "", "A" * 33], [1] * 6, 2)
    assert r2["degree"].tolist() == [2, 2, 2, 0, 0, 0] and st2["edges"] == 3
    # a rotation: Hamming 12, Levenshtein 2
    s = "ACDEFGHIKLMN"
    assert clu.lev(s.encode(), (s[1:] + s[0]).encode()) == 2
    assert clu.expected_lev_network([0, 0], [s, s[1:] + s[0]], [1, 1], 1)[1]["edges"] == 0
    assert clu.expected_lev_network([0, 0], [s, s[1:] + s[0]], [1, 1], 2)[1]["edges"] == 1
    assert cnu.expected_network([0, 0], [s, s[1:] + s[0]], [1, 1], 2)[1]["edges"] == 0
    # the symmetric-deletion search against all pairs by the DP
    strings = clu.families_indel(400, seed=3, length=9)
    for D in (1, 2):
        r, st = clu.expected_lev_network([k % 2 for k in range(400)], strings, [1] * 400, D)
        want = {(a, b) for a in range(400) for b in range(a + 1, 400)
                if a % 2 == b % 2 and clu.lev(strings[a].encode(), strings[b].encode()) <= D}
        got = {(a, int(b)) for a in range(400) for b in r["adj"][int(r["adj_off"][a]):int(r["adj_off"][a + 1])] if a < b}
        assert got == want and len(want) > 100
        two, extra = clu.edge_kinds(strings, r, D)
        assert two > 30 and (D == 1 or extra > 0)


def test_formatter_takes_edges_between_two_lengths():
    strings = ["CASSF", "CASSFF", "CASSY", "ASSF", "CASSF"]
    result, _ = clu.expected_lev_network([0] * 5, strings, [1] * 5, 2)
    off, text = cnu.node_text(strings)
    got = nat.format_cdr3_edges(off, text, result, metric="levenshtein").decode()
    assert got == clu.edges_text(strings, result)
    assert got == "a\tb\tdistance\n0\t1\t1\n0\t2\t1\n0\t3\t1\n0\t4\t0\n1\t2\t2\n1\t3\t2\n1\t4\t1\n2\t3\t2\n2\t4\t1\n3\t4\t1\n"
    with pytest.raises(nat.DcrxError, match="two lengths"):      # the Hamming formatter still refuses them
        nat.format_cdr3_edges(off, text, result)
    ham, _ = cnu.expected_network([0] * 5, strings, [1] * 5, 2)
    assert nat.format_cdr3_edges(off, text, ham, metric="hamming") == nat.format_cdr3_edges(off, text, ham)
    with pytest.raises(nat.DcrxError, match="metric") as e:
        nat.format_cdr3_edges(off, text, ham, metric=2)
    assert e.value.code == -1
    with pytest.raises(ValueError, match="hamming, levenshtein"):
        nat.format_cdr3_edges(off, text, ham, metric="lev")


def test_new_entries_refuse_before_the_device_and_the_abi_version_stays():
    assert nat.ABI_VERSION == 5 == nat.lib().dcrx_abi_version()
    assert nat.CDR3_METRICS == {"hamming": 0, "levenshtein": 1}
    hdr = open(os.path.join(os.path.dirname(cu.__file__), "..", "include", "dcrx.h")).read()
    assert "#define DCRX_CDR3NET_HAMMING 0" in hdr and "#define DCRX_CDR3NET_LEVENSHTEIN 1" in hdr
    for name in ("dcrx_cdr3net_metric_work_bytes", "dcrx_cdr3_neighbours_metric_device", "dcrx_cdr3_network_metric",
                 "dcrx_format_cdr3_edges_metric"):
        assert name in nat.EXPORTS and hasattr(nat.lib(), name)
    assert nat.cdr3net_work_bytes(1 << 30, 0, metric="levenshtein") == 0 and nat.cdr3net_work_bytes(1000, 0, metric=2) == 0
    off, text = cnu.node_text(["CASSF", "CASSFF"])
    for bad in (0, 3):
        with pytest.raises(nat.DcrxError, match="1 or 2") as e:
            nat.cdr3_network([0, 0], off, text, [1, 1], bad, metric="levenshtein")
        assert e.value.code == -1
    with pytest.raises(nat.DcrxError, match="metric") as e:
        nat.cdr3_network([0, 0], off, text, [1, 1], 1, metric=7)
    assert e.value.code == -1
    back = off.copy()
    back[1] = 99
    with pytest.raises(nat.DcrxError, match="backwards"):
        nat.cdr3_network([0, 0], back, text, [1, 1], 1, metric="levenshtein")
    # no node: nothing is launched
    e_off, e_text = cnu.node_text([])
    cnu.assert_same(nat.cdr3_network([], e_off, e_text, [], 2, want_edges=True, metric="levenshtein"), clu.expected_lev_network([], [], [], 2))


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
    monkeypatch.setattr(nat, "cdr3_network", clu.brute_force_native(calls))
    ot = gu.oracle_tables(ts)
    monkeypatch.setattr(nat, "decombine", lambda tables, batch, orientation="reverse", allow_ns=False, lenthreshold=130, flags=0:
                        pu.oracle_records(ot, nat.unpack_reads(batch), orientation, allow_ns, lenthreshold))
    monkeypatch.setattr(nat, "umi_neighbours", ccu.brute_neighbours)
    nu.OracleCountDevice(monkeypatch)
    common = ["-tfdir", "tags", "-tg", ts["tags"], "-sp", ts["species"], "-c", ts["chain"]]
    return fx, G, calls, common


def _clonotype_columns(text: str):
    rows = [ln.split("\t") for ln in text.splitlines()[1:]]
    return [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [int(r[3]) for r in rows]


def _want(clonotypes_text: str, mode: str, D: int):
    """(clusters text, edges text, statistics, result) under the Levenshtein metric for the clonotype table a run wrote."""
    v, j, aa, dup = _clonotype_columns(clonotypes_text)
    result, stats = clu.expected_lev_network(cnu.call_classes(v, j, mode), aa, dup, D)
    return cnu.file_text(v, j, aa, dup, result), clu.edges_text(aa, result), stats, result


@pytest.mark.parametrize("mode,D", [("none", 2), ("v", 1)])
def test_pipeline_writes_the_levenshtein_files(coding, tmp_path, mode, D, capsys):
    fx, G, calls, common = coding
    pipeline.main(["pipeline", "-in", "COD_1.fq", "-br", "R2", "-nbc", "--count-dcrs", "--clonotypes", "--cdr3-network", "--write-cdr3-edges",
                   "--cdr3-metric", "levenshtein", "--cdr3-class", mode, "--cdr3-distance", str(D), "-dc", "-s", "-dz"] + common)
    clon = (tmp_path / "dcr_COD_1_beta.clonotypes.tsv").read_text()
    want, want_edges, stats, result = _want(clon, mode, D)
    assert (tmp_path / "dcr_COD_1_beta.cdr3_clusters.tsv").read_text() == want
    assert (tmp_path / "dcr_COD_1_beta.cdr3_edges.tsv").read_text() == want_edges
    assert translate.chain_cdr3_network_stats["b"] == translate.cdr3_network_stats == stats
    assert len(calls) == 1 and calls[0][2:] == (D, True, {"metric": "levenshtein"})
    assert "CDR3 network metric: levenshtein" in capsys.readouterr().out
    if mode == "none":
        aa = _clonotype_columns(clon)[2]
        assert clu.edge_kinds(aa, result, D)[0] > 0      # (the fixture has neighbours of two lengths to find)
        assert stats["edges"] > cnu.expected_network([0] * len(aa), aa, [1] * len(aa), D)[1]["edges"]


def test_without_the_flag_nothing_changes(coding, tmp_path, capsys, monkeypatch):
    """No --cdr3-metric, and --cdr3-metric hamming: the call carries no `metric` keyword (what stands in for the native function
    in the existing tests does not know it), the files are the Hamming ones byte for byte, and no line is added."""
    fx, G, calls, common = coding
    base = ["pipeline", "-in", "COD_1.fq", "-br", "R2", "-nbc", "--count-dcrs", "--clonotypes", "--cdr3-network", "--write-cdr3-edges",
            "--cdr3-class", "none", "--cdr3-distance", "2", "-dc", "-s", "-dz"] + common
    old_stand_in = cnu.brute_force_native()      # the stand-in of the existing tests: no `metric` keyword at all
    monkeypatch.setattr(nat, "cdr3_network", lambda *a, **k: (calls.append(dict(k)), old_stand_in(*a, **k))[1])
    pipeline.main(base)
    plain_out = capsys.readouterr().out
    files = {n: (tmp_path / n).read_bytes() for n in ("dcr_COD_1_beta.cdr3_clusters.tsv", "dcr_COD_1_beta.cdr3_edges.tsv")}
    pipeline.main(base + ["--cdr3-metric", "hamming"])
    named_out = capsys.readouterr().out
    assert calls == [{"want_edges": True}, {"want_edges": True}]
    v, j, aa, dup = _clonotype_columns((tmp_path / "dcr_COD_1_beta.clonotypes.tsv").read_text())
    result, _ = cnu.expected_network([0] * len(aa), aa, dup, 2)
    assert files["dcr_COD_1_beta.cdr3_clusters.tsv"].decode() == cnu.file_text(v, j, aa, dup, result)
    assert files["dcr_COD_1_beta.cdr3_edges.tsv"].decode() == cnu.edges_text(aa, result)
    for n, text in files.items():
        assert (tmp_path / n).read_bytes() == text
    assert "metric" not in plain_out and "metric" not in named_out

    def steady(out):      # (the last line carries the run's duration)
        return [ln for ln in out.splitlines() if not ln.startswith("Pipeline complete in")]
    assert steady(plain_out) == steady(named_out)


def test_translate_gzipped_and_dontsave(coding, tmp_path):
    fx, G, calls, common = coding
    pipeline.main(["pipeline", "-in", "COD_1.fq", "-br", "R2", "-nbc", "--count-dcrs", "--clonotypes", "-dc", "-s", "-dz"] + common)
    clon = (tmp_path / "dcr_COD_1_beta.clonotypes.tsv").read_text()
    assert calls == []
    tr = ["translate", "-in", "dcr_COD_1_beta.nbc", "-nbc", "--count-dcrs", "--clonotypes", "--cdr3-network", "--cdr3-metric", "levenshtein"] + common
    pipeline.main(tr)
    want, _, stats, _ = _want(clon, "v", 1)
    assert gzip.open(tmp_path / "dcr_COD_1_beta.cdr3_clusters.tsv.gz", "rt").read() == want
    assert not (tmp_path / "dcr_COD_1_beta.cdr3_edges.tsv.gz").exists() and translate.cdr3_network_stats == stats
    assert calls[-1][2:] == (1, False, {"metric": "levenshtein"})
    # dontsave: the statistics, no file
    os.mkdir(tmp_path / "none")
    pipeline.main(["pipeline", "-in", "COD_1.fq", "-br", "R2", "-nbc", "--count-dcrs", "--clonotypes", "--cdr3-network", "--cdr3-metric",
                   "levenshtein", "-dc", "-s", "-ds", "-op", "none" + os.sep] + common)
    assert not [x for x in os.listdir(tmp_path / "none") if "cdr3" in x] and translate.cdr3_network_stats == stats


def test_two_chains_write_their_own_files(tmp_path, monkeypatch):
    """`pipeline -c a,b ... --cdr3-network --cdr3-metric levenshtein --write-cdr3-edges`: each chain's files equal its
    single-chain run's."""
    monkeypatch.chdir(tmp_path)
    nu.OracleCountDevice(monkeypatch)
    ta, tb = synth.config3_tagsets()
    sets = {"a": ta, "b": tb}
    infos = {c: cu.coding_genes(40 + k, len(ts.v_regions), len(ts.j_regions)) for k, (c, ts) in enumerate(sets.items())}
    monkeypatch.setattr(translate, "import_gene_information", lambda inputargs: infos[inputargs["chain"]])
    monkeypatch.setattr(nat, "clonotypes", lambda genes, counted: cu.brute_force_native(translate._genes)(genes, counted))
    calls = []
    monkeypatch.setattr(nat, "cdr3_network", clu.brute_force_native(calls))
    reads = nu.clonal_reads(ta, 300, seed=31) + nu.clonal_reads(tb, 300, seed=32)
    ta.write(str(tmp_path / "tags"))
    tb.write(str(tmp_path / "tags"))
    nu.write_fastq(tmp_path / "NBC_1.fq", reads)
    base = ["pipeline", "-in", "NBC_1.fq", "-br", "R2", "-nbc", "--count-dcrs", "--clonotypes", "--cdr3-network", "--write-cdr3-edges",
            "--cdr3-metric", "levenshtein", "--cdr3-class", "none", "--cdr3-distance", "2", "-tfdir", "tags", "-tg", ta.tags, "-sp", ta.species,
            "-dc", "-s", "-dz"]
    names = [f"dcr_NBC_1_{n}.{kind}.tsv" for n in ("alpha", "beta") for kind in ("cdr3_clusters", "cdr3_edges", "clonotypes")]
    pipeline.main(base + ["-c", "a,b"])
    both = {n: (tmp_path / n).read_text() for n in names}
    stats = {c: dict(translate.chain_cdr3_network_stats[c]) for c in "ab"}
    assert [c[4] for c in calls] == [{"metric": "levenshtein"}] * 2
    for c, chain in (("a", "alpha"), ("b", "beta")):
        for n in names:
            os.remove(tmp_path / n) if chain in n else None
        pipeline.main(base + ["-c", c])
        for n in names:
            if chain in n:
                assert (tmp_path / n).read_text() == both[n], n
        assert translate.cdr3_network_stats == stats[c] and stats[c]["nodes_in"] > 3
        want, want_edges, _, _ = _want(both[f"dcr_NBC_1_{chain}.clonotypes.tsv"], "none", 2)
        assert both[f"dcr_NBC_1_{chain}.cdr3_clusters.tsv"] == want and both[f"dcr_NBC_1_{chain}.cdr3_edges.tsv"] == want_edges
    assert both[names[0]] != both[names[3]]


def test_refusals_before_anything_is_read(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(nat, "FastqReader", lambda *a, **k: pytest.fail("a reader was opened"))
    monkeypatch.setattr(translate, "import_gene_information", lambda *a, **k: pytest.fail("gene files were read"))
    monkeypatch.setattr(nat, "clonotypes", lambda *a, **k: pytest.fail("the device was called"))
    monkeypatch.setattr(nat, "cdr3_network", lambda *a, **k: pytest.fail("the device was called"))
    monkeypatch.setattr(gzip, "open", lambda *a, **k: pytest.fail("a file was opened"))
    pl = ["pipeline", "-in", "X_1.fq", "-br", "R2", "-c", "b", "-tfdir", "tags", "-nbc", "--count-dcrs"]
    tr = ["translate", "-in", "dcr_X_1_beta.nbc.gz", "-c", "b", "-nbc", "--count-dcrs"]
    for argv in (pl + ["--clonotypes", "--cdr3-metric", "levenshtein"],                       # without --cdr3-network
                 tr + ["--clonotypes", "--cdr3-metric", "hamming"],
                 pl + ["--cdr3-metric", "levenshtein"],
                 pl + ["--cdr3-network", "--cdr3-metric", "levenshtein"],                     # no clonotype table
                 pl + ["--clonotypes", "--cdr3-network", "--cdr3-metric", "edit"],            # a metric that does not exist
                 tr + ["--clonotypes", "--cdr3-network", "--cdr3-metric", "levenshtein", "--cdr3-distance", "3"]):
        with pytest.raises(SystemExit) as e:
            pipeline.main(argv)
        assert e.value.code == 2, argv
    assert os.listdir(tmp_path) == []
    args = dio.create_args_dict(infile="X_1.fq", chain="b", bc_read="R2", tagfastadir="tags", outpath="", command="pipeline", nobarcoding=True,
                                count_dcrs=True, clonotypes=True, cdr3_network=True, cdr3_metric="levenshtein")
    assert args["cdr3_metric"] == "levenshtein" and pipeline.cdr3_network_refusal(args) is None
    assert dio.create_args_dict(infile="x", chain="b", bc_read="R2")["cdr3_metric"] is None
    assert "hamming or levenshtein" in pipeline.cdr3_network_refusal(dict(args, cdr3_metric="edit"))
    with pytest.raises(ValueError, match="hamming or levenshtein"):
        pipeline.run(dict(args, cdr3_metric="edit"))
    c = dio.cli_args(["translate", "-in", "x.freq"])
    assert c["cdr3_metric"] is None and c["cdr3_options_given"] == []
    c = dio.cli_args(["translate", "-in", "x.freq", "--cdr3-metric", "levenshtein"])
    assert c["cdr3_metric"] == "levenshtein" and c["cdr3_options_given"] == ["--cdr3-metric"]
    assert "--cdr3-metric belongs to --cdr3-network" in pipeline.cdr3_network_refusal(c)
