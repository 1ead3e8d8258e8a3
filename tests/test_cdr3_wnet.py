"""`--cdr3-network --cdr3-metric weighted` (include/dcrx.h "the CDR3 network, weighted") without a GPU: every refusal of the four C
entries and of the stage, the symbols exported, the old entries' refusal of metric 2, the host walk of the kernel's steps
(tests/host_cdr3wnet) against the contract in Python (tests/cdr3_wnet_util.py) on the constructed lists, the host formatter, the
stage over a stubbed native call, and the stand-alone sanitizer run of the host walk."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import io as dio
from decombinator_amd import match as mt
from decombinator_amd import pipeline, translate
from tests import cdr3_network_util as cnu
from tests import cdr3_wmatch_util as wu
from tests import cdr3_wnet_util as nu
from tests.test_cdr3_lev import _clonotype_columns, coding      # noqa: F401 (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- refusals of the C entries: on the host, before any device call ----

def _bad_costs():
    ok = nat.Cdr3Cost.default()
    asym, diag = ok.sub.copy(), ok.sub.copy()
    asym[1, 3] = 5
    diag[26, 26] = 1
    return [(nat.Cdr3Cost(asym), 24, "not symmetric"), (nat.Cdr3Cost(diag), 24, "not zero on its diagonal"),
            (nat.Cdr3Cost.default(gap=0), 24, "the gap cost is 1 .. 255"), (nat.Cdr3Cost.default(gap=256), 24, "the gap cost is 1 .. 255"),
            (nat.Cdr3Cost.default(ntrim=17), 24, "a trim is 0 .. 16"), (nat.Cdr3Cost.default(ctrim=17), 24, "a trim is 0 .. 16"),
            (ok, 65536, "the radius is 0 .. 65535"), (None, 24, "null cost")]


def test_the_weighted_entries_refuse_what_the_contract_refuses():
    off, text = cnu.node_text(["CASSF", "CASSFF"])
    for cost, radius, msg in _bad_costs():
        with pytest.raises(nat.DcrxError, match="dcrx_cdr3_network_weighted: .*" + msg) as e:
            nat.cdr3_network_weighted([0, 0], off, text, [1, 1], cost, radius)
        assert e.value.code == -1
        with pytest.raises(nat.DcrxError, match="dcrx_cdr3_neighbours_weighted_device: .*" + msg) as e:
            nat.cdr3_neighbours_weighted_device(0, None, None, None, 0, cost, radius, None, None, None, None, 0, None, None, 0)
        assert e.value.code == -1
        if radius <= 65535:      # (the formatter takes no radius)
            with pytest.raises(nat.DcrxError, match="dcrx_format_cdr3_edges_weighted: .*" + msg):
                nat.format_cdr3_edges_weighted(off, text, {"adj_off": np.zeros(3, np.uint64), "adj": []}, cost)
    ok = nat.Cdr3Cost.default()
    assert nat.cdr3net_weighted_work_bytes(1 << 30, 0) == 0
    with pytest.raises(nat.DcrxError, match="2\\^30 or more nodes") as e:
        nat.cdr3_neighbours_weighted_device(1 << 30, None, None, None, 0, ok, 24, None, None, None, None, 0, None, None, 0)
    assert e.value.code == nat.E_UNSUPPORTED
    L = nat.lib()
    c = ok.as_c()
    assert L.dcrx_cdr3_network_weighted(1 << 30, None, None, None, None, C.addressof(c), 24, None, None, None, None, None, None, None, None, 0,
                                        None, None) == nat.E_UNSUPPORTED
    back = off.copy()
    back[1] = 99
    with pytest.raises(nat.DcrxError, match="dcrx_cdr3_network_weighted: offsets go backwards"):
        nat.cdr3_network_weighted([0, 0], back, text, [1, 1], ok, 24)
    assert L.dcrx_cdr3_network_weighted(2, None, None, None, None, C.addressof(c), 24, None, None, None, None, None, None, None, None, 0, None,
                                        None) == -1 and b"null argument" in L.dcrx_last_error()
    # the table's unread rows and columns may hold anything; the limits themselves pass; no node: nothing is launched
    loose = nat.Cdr3Cost.default(gap=255, ntrim=16, ctrim=16)
    loose.sub[0, 5], loose.sub[27, 1], loose.sub[3, 31] = 9, 8, 7
    e_off, e_text = cnu.node_text([])
    nu.assert_same(nat.cdr3_network_weighted([], e_off, e_text, [], loose, 65535, want_edges=True), nu.wanted("no_nodes"))
    nat.cdr3_neighbours_weighted_device(0, None, None, None, 0, loose, 65535, None, None, None, None, 0, None, None, 0)
    # an edge the metric cannot have: a byte outside A .. Z, a string out of reach
    for strings in (["CASSF", "CASsF"], ["CASSF", "C" * 33]):
        o, t = cnu.node_text(strings)
        with pytest.raises(nat.DcrxError, match="reach"):
            nat.format_cdr3_edges_weighted(o, t, {"adj_off": np.array([0, 1, 2], np.uint64), "adj": np.array([1, 0], np.uint32)}, ok)


def test_exports_and_abi():
    hdr = open(os.path.join(ROOT, "include", "dcrx.h")).read()
    assert "#define DCRX_ABI_VERSION 5" in hdr and "the CDR3 network, weighted" in hdr
    for name in ("dcrx_cdr3net_weighted_work_bytes", "dcrx_cdr3_neighbours_weighted_device", "dcrx_cdr3_network_weighted",
                 "dcrx_format_cdr3_edges_weighted"):
        assert name in nat.EXPORTS and name + "(" in hdr and hasattr(nat.lib(), name)
    for name in ("cdr3net_weighted_work_bytes", "cdr3_neighbours_weighted_device", "cdr3_network_weighted", "format_cdr3_edges_weighted"):
        assert callable(getattr(nat, name))


def test_the_old_entries_still_refuse_metric_2():
    L = nat.lib()
    assert nat.CDR3_METRICS == {"hamming": 0, "levenshtein": 1} and nat.CDR3_METRIC_WEIGHTED == 2
    assert L.dcrx_cdr3net_metric_work_bytes(10, 0, 2) == 0
    off, text = cnu.node_text(["CASSF", "CASSFF"])
    with pytest.raises(nat.DcrxError, match="the metric is DCRX_CDR3NET_HAMMING or DCRX_CDR3NET_LEVENSHTEIN") as e:
        nat.cdr3_network([0, 0], off, text, [1, 1], 1, metric=2)
    assert e.value.code == -1
    assert L.dcrx_cdr3_neighbours_metric_device(0, None, None, None, 0, 1, 2, None, None, None, 0, None, None, 0, None) == -1
    assert b"metric" in L.dcrx_last_error()
    with pytest.raises(nat.DcrxError, match="metric"):
        nat.format_cdr3_edges(off, text, {"adj_off": np.zeros(3, np.uint64), "adj": []}, metric=2)
    with pytest.raises(ValueError, match="metric"):
        nat.cdr3_metric_code("weighted")


# ---- the host walk of the kernel's steps ----

def test_host_walk_gives_the_contract_on_the_constructed_lists():
    lists = nu.constructed()
    assert sorted(lists) == sorted(nu.NAMES)
    blocks = {(len(nodes) + 255) // 256 for nodes, _, _, _ in lists.values()}
    assert {1, 3, 6} <= blocks      # grids of 1, 3 and 6 blocks
    for name, (nodes, cost, R, _) in lists.items():
        want, _ = nu.wanted(name)
        degree, adj_off, adj, adj_dist = nu.host_network(nodes, cost, R)
        for k, got in (("degree", degree), ("adj_off", adj_off), ("adj", adj), ("adj_dist", adj_dist)):
            assert np.array_equal(np.asarray(got, np.uint64), np.asarray(want[k], np.uint64)), (name, k)
        assert nu.symmetric(want)


def test_the_symmetry_pairs_on_the_host_walk():
    """Every pair (L, L + d) with the best gap place first, last and inside: each node's row holds the other, and both carry the
    pair's one distance — the shorter string's lane and the longer string's lane run two code paths of weighted_within."""
    for trims in ((3, 2), (0, 0)):
        nodes, cost, R, pairs = nu.symmetry(*trims)
        degree, adj_off, adj, adj_dist = nu.host_network(nodes, cost, R)
        for short, long_, d, place in pairs:
            for i, j in ((short, long_), (long_, short)):
                assert adj[int(adj_off[i]):int(adj_off[i + 1])].tolist() == [j], (trims, short, long_, d, place)
                assert adj_dist[int(adj_off[i])] == d * cost.gap == wu.dist(nodes.strings[i], nodes.strings[j], cost)


def test_the_numpy_form_is_the_literal_one():
    for name in ("symmetry_3_2", "class_bits_1", "trim_16_16", "cells_255_one_below"):
        nodes, cost, R, _ = nu.constructed()[name]
        nu.assert_same(nu.expected_numpy(nodes, cost, R), nu.expected(nodes, cost, R), name)
    nodes = nu.planted(400, 3, seed=2)
    want = nu.expected(nodes, wu.default_cost(), 24)
    assert want[1]["edges"] > 30 and len(set(want[0]["adj_dist"].tolist())) > 3
    nu.assert_same(nu.expected_numpy(nodes, wu.default_cost(), 24), want)


def test_sanitizer_run_of_the_host_walk():
    """The stand-alone program (its own main) under AddressSanitizer and UBSan: host code, on the CPU."""
    got = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "host_cdr3wnet"), "asan"], capture_output=True, text=True)
    assert got.returncode == 0, got.stdout[-2000:] + got.stderr[-2000:]
    assert got.stdout.strip().endswith("ok") and "rows differ" in got.stdout and "non-letters on the tile edges" in got.stdout


# ---- the host formatter ----

def test_format_cdr3_edges_weighted_against_python():
    for name in ("symmetry_3_2", "random_table", "cells_255_R65535", "reach"):
        nodes, cost, R, _ = nu.constructed()[name]
        result, stats = nu.wanted(name)
        off, text = cnu.node_text(nodes.strings)
        got = nat.format_cdr3_edges_weighted(off, text, result, cost)
        assert got.decode() == nu.edges_text(nodes.strings, result, cost)
        lines = got.splitlines()[1:]
        assert len(lines) == stats["edges"] > 0
        # the host's literal minimum is the distance the contract gives every adjacency entry
        dist = {}
        for i in range(len(nodes)):
            for k in range(int(result["adj_off"][i]), int(result["adj_off"][i + 1])):
                dist[(i, int(result["adj"][k]))] = int(result["adj_dist"][k])
        assert all(dist[(int(a), int(b))] == int(d) for a, b, d in (ln.split(b"\t") for ln in lines))
    e_off, e_text = cnu.node_text([])
    assert nat.format_cdr3_edges_weighted(e_off, e_text, {"adj_off": np.zeros(1, np.uint64), "adj": []}, wu.default_cost()) == b"a\tb\tdistance\n"


# ---- the stage ----

BASE = ["pipeline", "-in", "COD_1.fq", "-br", "R2", "-nbc", "--count-dcrs", "--clonotypes", "-dc", "-s", "-dz"]


def _want(clon: str, mode: str, cost, R: int):
    v, j, aa, dup = _clonotype_columns(clon)
    nodes = nu.Nodes(cnu.call_classes(v, j, mode), aa, dup)
    result, stats = nu.expected(nodes, cost, R)
    not_letters = sum(1 <= len(s) <= 32 and not wu.letters(s) for s in nodes.strings)
    return cnu.file_text(v, j, aa, dup, result), nu.edges_text(aa, result, cost), stats, not_letters


@pytest.mark.parametrize("flags,settings,mode", [([], (24, 12, 3, 2), "v"),
                                                 (["--cdr3-radius", "30", "--cdr3-gap-cost", "9", "--cdr3-trim", "2,1", "--cdr3-class", "none"],
                                                  (30, 9, 2, 1), "none")])
def test_the_stage_over_a_stubbed_native_call(coding, tmp_path, monkeypatch, capsys, flags, settings, mode):
    fx, G, calls, common = coding
    wcalls = []
    monkeypatch.setattr(nat, "cdr3_network_weighted", nu.brute_force_native(wcalls))
    pipeline.main(BASE + ["--cdr3-network", "--write-cdr3-edges", "--cdr3-metric", "weighted"] + flags + common)
    R, gap, ntrim, ctrim = settings
    cost = wu.default_cost(gap, ntrim, ctrim)
    clon = (tmp_path / "dcr_COD_1_beta.clonotypes.tsv").read_text()
    want, want_edges, stats, not_letters = _want(clon, mode, cost, R)
    assert (tmp_path / "dcr_COD_1_beta.cdr3_clusters.tsv").read_text() == want
    assert (tmp_path / "dcr_COD_1_beta.cdr3_edges.tsv").read_text() == want_edges
    assert stats["edges"] > 0 and want_edges.count("\n") == stats["edges"] + 1
    assert calls == [] and len(wcalls) == 1 and wcalls[0][3:] == (R, True)
    sent = wcalls[0][2]
    assert (sent.gap, sent.ntrim, sent.ctrim) == (gap, ntrim, ctrim) and (sent.sub == nat.Cdr3Cost.default_table()).all()
    assert translate.cdr3_network_stats == dict(stats, not_letters=not_letters) == translate.chain_cdr3_network_stats["b"]
    out = capsys.readouterr().out.splitlines()
    at = out.index(f"CDR3 network metric: weighted (radius {R}, gap {gap}, trim {ntrim},{ctrim}; linked CDR3s may differ in length)")
    assert out[at + 1] == (f"CDR3 network: {stats['nodes_in']:,} clonotypes in ({stats['out_of_reach']:,} out of reach); {stats['edges']:,} "
                           f"pairs within radius {R}; {stats['clusters_out']:,} clusters, {stats['singletons']:,} of them single (the "
                           f"largest holds {stats['largest_cluster']:,}; at most {stats['largest_degree']:,} neighbours)")
    assert out[at + 2] == f"CDR3 network: {not_letters:,} clonotypes took no part for a byte outside A..Z"


def test_a_matrix_file_reaches_the_call_and_translate_runs_the_stage(coding, tmp_path, monkeypatch):
    fx, G, calls, common = coding
    wcalls = []
    monkeypatch.setattr(nat, "cdr3_network_weighted", nu.brute_force_native(wcalls))
    letters = nat.AMINO_ACIDS
    cell = lambda x, y: 0 if x == y else 1 + (ord(x) * ord(y)) % 23
    rows = ["\t".join(["."] + list(letters))] + ["\t".join([x] + [str(cell(x, y)) for y in letters]) for x in letters]
    (tmp_path / "m.tsv").write_text("\n".join(rows) + "\n")
    pipeline.main(BASE + common)
    clon = (tmp_path / "dcr_COD_1_beta.clonotypes.tsv").read_text()
    pipeline.main(["translate", "-in", "dcr_COD_1_beta.nbc", "-nbc", "--count-dcrs", "--clonotypes", "--cdr3-network", "--cdr3-metric", "weighted",
                   "--cdr3-cost-matrix", "m.tsv", "--cdr3-radius", "40", "-dz"] + common)
    cost = nat.Cdr3Cost.from_file(str(tmp_path / "m.tsv"))
    assert len(wcalls) == 1 and wcalls[0][3:] == (40, False) and (wcalls[0][2].sub == cost.sub).all()
    want, _, stats, _ = _want(clon, "v", cost, 40)
    assert (tmp_path / "dcr_COD_1_beta.cdr3_clusters.tsv").read_text() == want and stats["edges"] > 0
    assert not (tmp_path / "dcr_COD_1_beta.cdr3_edges.tsv").exists()


def test_without_the_flag_the_new_call_is_not_made(coding, tmp_path, monkeypatch, capsys):
    fx, G, calls, common = coding
    monkeypatch.setattr(nat, "cdr3_network_weighted", lambda *a, **k: pytest.fail("weighted without the flag"))
    monkeypatch.setattr(nat, "format_cdr3_edges_weighted", lambda *a, **k: pytest.fail("weighted without the flag"))
    for metric in ([], ["--cdr3-metric", "levenshtein"]):
        pipeline.main(BASE + ["--cdr3-network", "--write-cdr3-edges"] + metric + common)
    assert [c[4] for c in calls] == [{}, {"metric": "levenshtein"}]
    out = capsys.readouterr().out
    assert "weighted" not in out and "radius" not in out and "A..Z" not in out


REFUSALS = [
    (["--cdr3-radius", "24"], "--cdr3-radius belongs to --cdr3-network"),
    (["--cdr3-gap-cost", "12", "--clonotypes"], "--cdr3-gap-cost belongs to --cdr3-network"),
    (["--cdr3-trim", "3,2"], "--cdr3-trim belongs to --cdr3-network"),
    (["--cdr3-cost-matrix", "m.tsv"], "--cdr3-cost-matrix belongs to --cdr3-network"),
    (["--clonotypes", "--cdr3-network", "--cdr3-radius", "24"], "--cdr3-radius goes with --cdr3-metric weighted"),
    (["--clonotypes", "--cdr3-network", "--cdr3-metric", "levenshtein", "--cdr3-gap-cost", "12"], "--cdr3-gap-cost goes with --cdr3-metric weighted"),
    (["--clonotypes", "--cdr3-network", "--cdr3-metric", "hamming", "--cdr3-trim", "3,2"], "--cdr3-trim goes with --cdr3-metric weighted"),
    (["--clonotypes", "--cdr3-network", "--cdr3-cost-matrix", "m.tsv"], "--cdr3-cost-matrix goes with --cdr3-metric weighted"),
    (["--clonotypes", "--cdr3-network", "--cdr3-metric", "weighted", "--cdr3-distance", "2"], "--cdr3-distance does not apply"),
    (["--clonotypes", "--cdr3-network", "--cdr3-metric", "weighted", "--cdr3-distance", "1"], "--cdr3-distance does not apply"),
    (["--clonotypes", "--cdr3-network", "--cdr3-metric", "weighted", "--cdr3-radius", "65536"], "--cdr3-radius is 0 to 65535"),
    (["--clonotypes", "--cdr3-network", "--cdr3-metric", "weighted", "--cdr3-radius", "-1"], "--cdr3-radius is 0 to 65535"),
    (["--clonotypes", "--cdr3-network", "--cdr3-metric", "weighted", "--cdr3-trim", "17,2"], "--cdr3-trim is N,C"),
    (["--clonotypes", "--cdr3-network", "--cdr3-metric", "weighted", "--cdr3-trim", "3,17"], "--cdr3-trim is N,C"),
    (["--clonotypes", "--cdr3-network", "--cdr3-metric", "weighted", "--cdr3-trim", "3"], "--cdr3-trim is N,C"),
    (["--clonotypes", "--cdr3-network", "--cdr3-metric", "weighted", "--cdr3-gap-cost", "0"], "--cdr3-gap-cost is 1 to 255"),
    (["--clonotypes", "--cdr3-network", "--cdr3-metric", "weighted", "--cdr3-gap-cost", "256"], "--cdr3-gap-cost is 1 to 255"),
    (["--cdr3-network", "--cdr3-metric", "weighted"], "it needs --clonotypes"),
]


def _nothing_is_read(monkeypatch):
    import gzip
    monkeypatch.setattr(nat, "FastqReader", lambda *a, **k: pytest.fail("a reader was opened"))
    monkeypatch.setattr(translate, "import_gene_information", lambda *a, **k: pytest.fail("gene files were read"))
    monkeypatch.setattr(nat, "clonotypes", lambda *a, **k: pytest.fail("the device was called"))
    monkeypatch.setattr(nat, "cdr3_network", lambda *a, **k: pytest.fail("the device was called"))
    monkeypatch.setattr(nat, "cdr3_network_weighted", lambda *a, **k: pytest.fail("the device was called"))
    monkeypatch.setattr(gzip, "open", lambda *a, **k: pytest.fail("a file was opened"))


@pytest.mark.parametrize("extra,msg", REFUSALS)
def test_refusals_before_anything_is_read(tmp_path, monkeypatch, capsys, extra, msg):
    monkeypatch.chdir(tmp_path)
    _nothing_is_read(monkeypatch)
    for argv in (["pipeline", "-in", "X_1.fq", "-br", "R2", "-c", "b", "-tfdir", "tags", "-nbc", "--count-dcrs"],
                 ["translate", "-in", "dcr_X_1_beta.nbc.gz", "-c", "b", "-nbc", "--count-dcrs"]):
        with pytest.raises(SystemExit) as e:
            pipeline.main(argv + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, argv
    assert os.listdir(tmp_path) == []


def test_refusals_of_a_dictionary_and_of_a_bad_matrix_file(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    _nothing_is_read(monkeypatch)
    args = dio.create_args_dict(infile="X_1.fq", chain="b", bc_read="R2", tagfastadir="tags", outpath="", command="pipeline", nobarcoding=True,
                                count_dcrs=True, clonotypes=True, cdr3_network=True, cdr3_metric="weighted")
    assert [args[k] for k in ("cdr3_radius", "cdr3_gap_cost", "cdr3_trim", "cdr3_cost_matrix")] == [None] * 4
    assert pipeline.cdr3_network_refusal(args) is None
    assert pipeline.cdr3_network_refusal(dict(args, cdr3_radius=36, cdr3_gap_cost=8, cdr3_trim="4,3")) is None
    assert "hamming or levenshtein" in pipeline.cdr3_network_refusal(dict(args, cdr3_metric="tcrdist"))
    assert "weighted (with --cdr3-radius)" in pipeline.cdr3_network_refusal(dict(args, cdr3_metric="tcrdist"))
    assert "--cdr3-distance does not apply" in pipeline.cdr3_network_refusal(dict(args, cdr3_distance=2))
    assert "--cdr3-radius belongs to --cdr3-network" in pipeline.cdr3_network_refusal(dict(args, cdr3_network=False, cdr3_radius=5))
    assert "--cdr3-radius goes with" in pipeline.cdr3_network_refusal(dict(args, cdr3_metric=None, cdr3_radius=5))
    with pytest.raises(ValueError, match="--cdr3-radius is 0 to 65535"):
        pipeline.run(dict(args, cdr3_radius=70000))
    with pytest.raises(ValueError, match="hamming or levenshtein"):
        translate.cdr3_network(dict(args, cdr3_metric="tcrdist"), None)
    c = dio.cli_args(["translate", "-in", "x.freq", "--cdr3-metric", "weighted", "--cdr3-radius", "36", "--cdr3-gap-cost", "8", "--cdr3-trim", "4,3",
                      "--cdr3-cost-matrix", "m.tsv"])
    assert (c["cdr3_metric"], c["cdr3_radius"], c["cdr3_gap_cost"], c["cdr3_trim"], c["cdr3_cost_matrix"]) == ("weighted", 36, 8, "4,3", "m.tsv")
    assert c["cdr3_options_given"] == ["--cdr3-metric", "--cdr3-radius", "--cdr3-gap-cost", "--cdr3-trim", "--cdr3-cost-matrix"]
    c = dio.cli_args(["translate", "-in", "x.freq"])
    assert c["cdr3_options_given"] == [] and c["cdr3_radius"] is None
    # one parser of the four flags: match's
    cost, radius = mt.weighted_settings(dict(args))
    assert (radius, cost.gap, cost.ntrim, cost.ctrim) == (24, 12, 3, 2)
    # a bad matrix file: by its line, before the input is read
    good = "\n".join(["\t".join(["."] + list(nat.AMINO_ACIDS))] +
                     ["\t".join([x] + ["0" if x == y else "5" for y in nat.AMINO_ACIDS]) for x in nat.AMINO_ACIDS]) + "\n"
    (tmp_path / "m.tsv").write_text(good.replace("\nD\t5", "\nD\t6", 1))
    assert "line 4: D-A is 6 but A-D is 5" in pipeline.cdr3_network_refusal(dict(args, cdr3_cost_matrix="m.tsv"))
    with pytest.raises(SystemExit) as e:
        pipeline.main(["pipeline", "-in", "X_1.fq", "-br", "R2", "-c", "b", "-tfdir", "tags", "-nbc", "--count-dcrs", "--clonotypes", "--cdr3-network",
                       "--cdr3-metric", "weighted", "--cdr3-cost-matrix", "m.tsv"])
    assert e.value.code == 2 and "line 4: D-A is 6 but A-D is 5" in capsys.readouterr().err
    (tmp_path / "m.tsv").write_text(good)
    assert pipeline.cdr3_network_refusal(dict(args, cdr3_cost_matrix="m.tsv")) is None
