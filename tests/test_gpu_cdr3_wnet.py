"""`--cdr3-network --cdr3-metric weighted` through the HIP path: dcrx_cdr3_network_weighted against the contract written in Python
(tests/cdr3_wnet_util.py) — degrees, the CSR adjacency, every entry's distance, cluster_of, the cluster rows and the statistics,
exactly — on the constructed lists (small inputs, the symmetry pairs, tile and block edges, components, reach, costs), the
primitive's adjacency and work-space rules, one random table against the numpy form, and the sub-command's files."""
import ctypes as C
import gzip
import json
import os
import time

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import pipeline, synth, translate
from tests import cdr3_network_util as cnu
from tests import cdr3_wmatch_util as wu
from tests import cdr3_wnet_util as nu
from tests import clonotype_util as cu

pytestmark = pytest.mark.gpu


def _check(name):
    nodes, cost, R, _ = nu.constructed()[name]
    want = nu.wanted(name)
    got = nu.native(nodes, cost, R)
    nu.assert_same(got, want, name)
    nu.assert_same(nu.native(nodes, cost, R, want_edges=False), want, name)      # (the first call alone: no adjacency asked for)
    assert nu.symmetric(got[0])
    return got, want


def _names(*prefixes):
    return [n for n in nu.NAMES if n.startswith(prefixes)]


# ---- the constructed lists (each asserted its premise on the Python result when it was built) ----

@pytest.mark.parametrize("name", _names("no_", "one_", "equal_", "trimmed_", "conservative_"))
def test_small_inputs(name):
    _check(name)


@pytest.mark.parametrize("trims", [(3, 2), (0, 0)], ids=["trim-3-2", "trim-0-0"])
def test_both_lanes_of_a_pair_agree_on_its_distance(trims):
    """Pairs of lengths (L, L + d), the best gap place the first counted position, the last one and strictly inside: j is in i's
    row, i is in j's row, and both carry one distance, the contract's — the shorter string's lane reads the other string at i
    and i + d, the longer string's lane shifts its own words down by d bytes."""
    nodes, cost, R, pairs = nu.symmetry(*trims)
    (got, _), _ = _check(f"symmetry_{trims[0]}_{trims[1]}")
    off, adj, dist = got["adj_off"], got["adj"], got["adj_dist"]
    seen = set()
    for short, long_, d, place in pairs:
        for i, j in ((short, long_), (long_, short)):
            assert adj[int(off[i]):int(off[i + 1])].tolist() == [j], (short, long_, d, place)
            assert dist[int(off[i])] == wu.dist(nodes.strings[i], nodes.strings[j], cost) == d * cost.gap, (short, long_, d, place)
        seen.add((len(nodes.strings[short]), d))
    assert seen == {(L, d) for L in nu.SYM_LENGTHS for d in nu.SYM_GAPS if L + d <= 32}


@pytest.mark.parametrize("n", [255, 256, 257, 513, 1500])
def test_tile_and_block_edges(n):
    (got, stats), _ = _check(f"tiles_{n}")
    assert stats["edges"] > 10 * n


@pytest.mark.parametrize("name", _names("chain", "class_bits_"))
def test_components_and_classes(name):
    (got, stats), _ = _check(name)
    if name == "chain":
        assert got["cluster_of"].tolist() == [0, 0, 0] and got["adj_dist"].tolist() == [12, 12, 12, 12]


def test_nodes_out_of_reach_take_no_part():
    (got, stats), _ = _check("reach")
    out = sorted(set(nu.BAD_BYTES) | {300})
    assert all(got["degree"][i] == 0 and got["cluster_size"][got["cluster_of"][i]] == 1 for i in out)
    assert not (set(got["adj"].tolist()) & set(out)) and stats["out_of_reach"] == 1


@pytest.mark.parametrize("name", _names("cells_255_", "trim_", "random_table"))
def test_costs(name):
    (got, stats), _ = _check(name)
    assert name != "cells_255_R65535" or max(got["adj_dist"].tolist()) == 8160


# ---- the primitive ----

def _primitive(nodes, cost, R, work_bytes=None, adj_cap=None, pattern=0xA5, twice=False, dist=True):
    """dcrx_cdr3_neighbours_weighted_device over buffers and a stream of the caller's: (degree, adj_off, the whole adjacency and
    distance buffers, need, cap)."""
    m = len(nodes)
    off, text = cnu.node_text(nodes.strings)
    d_cls = nat.DeviceBuffer.from_host(np.asarray(nodes.classes, dtype=np.uint32))
    d_off = nat.DeviceBuffer.from_host(off)
    d_text = nat.DeviceBuffer.from_host(np.frombuffer(text + b"\0", np.uint8))
    d_deg, d_adj_off, d_need = nat.DeviceBuffer(max(16, m * 4)), nat.DeviceBuffer((m + 1) * 8), nat.DeviceBuffer(16)
    wb = nat.cdr3net_weighted_work_bytes(m, len(text)) if work_bytes is None else work_bytes
    assert wb > m * 32 or work_bytes is not None
    d_work = nat.DeviceBuffer(max(256, wb))
    stream = C.c_void_p()
    nat.check(nat.lib().dcrx_stream_create(C.byref(stream)))
    try:
        nat.cdr3_neighbours_weighted_device(m, d_cls, d_off, d_text, len(text), cost, R, d_deg, d_adj_off, None, None, 0, d_need, d_work, wb,
                                            stream)
        nat.check(nat.lib().dcrx_stream_synchronize(stream))
        need = int(d_need.to_host(np.uint64, 1)[0])
        cap = need if adj_cap is None else adj_cap(need)
        room = max(need, cap) + 64
        d_adj = nat.DeviceBuffer.from_host(np.full(room * 4, pattern, np.uint8))
        d_dist = nat.DeviceBuffer.from_host(np.full(room * 4, pattern, np.uint8))
        for _ in range(2 if twice else 1):      # two calls in a row on the caller's stream
            nat.cdr3_neighbours_weighted_device(m, d_cls, d_off, d_text, len(text), cost, R, d_deg, d_adj_off, d_adj, d_dist if dist else None,
                                                cap, d_need, d_work, wb, stream)
        nat.check(nat.lib().dcrx_stream_synchronize(stream))
    finally:
        nat.lib().dcrx_stream_destroy(stream)
    assert int(d_need.to_host(np.uint64, 1)[0]) == need
    return (d_deg.to_host(np.uint32, m), d_adj_off.to_host(np.uint64, m + 1), d_adj.to_host(np.uint32, room), d_dist.to_host(np.uint32, room),
            need, cap)


def test_primitive_work_space_and_adjacency_rules():
    nodes, cost, R, _ = nu.constructed()["tiles_1500"]
    want, stats = nu.wanted("tiles_1500")
    text_bytes = sum(len(s) for s in nodes.strings)
    assert nat.cdr3net_weighted_work_bytes(1 << 30, 0) == 0
    assert nat.cdr3net_weighted_work_bytes(1500, text_bytes) == nat.cdr3net_work_bytes(1500, text_bytes) > 0      # no presence masks
    assert nat.cdr3net_weighted_work_bytes(1500, text_bytes) < nat.cdr3net_work_bytes(1500, text_bytes, metric="levenshtein")
    with pytest.raises(nat.DcrxError, match="work space is smaller than dcrx_cdr3net_weighted_work_bytes") as e:
        _primitive(nodes, cost, R, work_bytes=nat.cdr3net_weighted_work_bytes(1500, text_bytes) - 1)
    assert e.value.code == -1
    filler = 0xA5A5A5A5
    deg, adj_off, adj, dist, need, cap = _primitive(nodes, cost, R, twice=True)
    assert need == cap == 2 * stats["edges"] == int(adj_off[-1])
    assert np.array_equal(deg, want["degree"]) and np.array_equal(adj_off, want["adj_off"])
    assert np.array_equal(adj[:need], want["adj"]) and np.array_equal(dist[:need], want["adj_dist"])
    assert (adj[need:] == filler).all() and (dist[need:] == filler).all()
    # no room, one short: the same need, nothing behind the cap is touched, every slot in front of it is right
    for short in (lambda n: 0, lambda n: n - 1):
        deg2, adj_off2, adj2, dist2, need2, cap2 = _primitive(nodes, cost, R, adj_cap=short)
        assert need2 == need and cap2 == short(need) and np.array_equal(deg2, deg) and np.array_equal(adj_off2, adj_off)
        assert (adj2[cap2:] == filler).all() and (dist2[cap2:] == filler).all()
        assert np.array_equal(adj2[:cap2], want["adj"][:cap2]) and np.array_equal(dist2[:cap2], want["adj_dist"][:cap2])
    # no distance buffer: the neighbours alone
    _, _, adj3, dist3, _, _ = _primitive(nodes, cost, R, dist=False)
    assert np.array_equal(adj3[:need], want["adj"]) and (dist3 == filler).all()
    # null and alignment refusals, as the other metrics' primitive
    buf = nat.DeviceBuffer(4096)
    with pytest.raises(nat.DcrxError, match="null argument"):
        nat.cdr3_neighbours_weighted_device(4, buf, buf, buf, 16, cost, R, None, buf, None, None, 0, None, buf, 4096)
    with pytest.raises(nat.DcrxError, match="null argument"):
        nat.cdr3_neighbours_weighted_device(4, buf, buf, buf, 16, cost, R, buf, buf, None, None, 8, None, buf, 4096)

    class Shifted:
        ptr = buf.ptr + 4
    with pytest.raises(nat.DcrxError, match="not 256-byte aligned"):
        nat.cdr3_neighbours_weighted_device(4, buf, buf, buf, 16, cost, R, buf, buf, None, None, 0, None, Shifted, 4000)


# ---- one random table ----

def test_random_table_equals_the_numpy_form_of_the_contract():
    """6 000 nodes in 20 classes at R = 24, a fifth of them planted near another node of their class; the reference (the literal
    minimum over every p, as array operations) takes 3.7 s on one CPU thread and is timed here."""
    nodes = nu.planted(6000, 20, seed=3)
    cost = wu.default_cost()
    t0 = time.perf_counter()
    want = nu.expected_numpy(nodes, cost, 24)
    print(f"reference: {time.perf_counter() - t0:.1f} s")
    result, stats = want
    assert stats["edges"] > 1000 and 100 < stats["clusters_out"] - stats["singletons"] and stats["largest_cluster"] > 3
    assert {0, 3, 6, 9, 12, 24} <= set(result["adj_dist"].tolist())
    off, adj = result["adj_off"], result["adj"]
    assert sum(len(nodes.strings[i]) != len(nodes.strings[j]) for i in range(len(nodes)) for j in adj[int(off[i]):int(off[i + 1])].tolist()) > 200
    got = nu.native(nodes, cost, 24)
    nu.assert_same(got, want)
    assert nu.symmetric(got[0])


# ---- the sub-command's files ----

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


@pytest.mark.parametrize("flags,settings", [([], (24, 12, 3, 2)),
                                            (["--cdr3-radius", "30", "--cdr3-gap-cost", "9", "--cdr3-trim", "2,1", "--write-cdr3-edges"], (30, 9, 2, 1))],
                         ids=["defaults", "radius-30-gap-9-trim-2-1-edges"])
def test_sub_command_byte_for_byte(flags, settings, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    fx, ts = _coding_workdir(tmp_path)
    base = ["pipeline", "-in", "COD_1.fq", "-br", "R2", "-nbc", "--count-dcrs", "--clonotypes", "-tfdir", "tags", "-tg", ts["tags"],
            "-sp", ts["species"], "-c", ts["chain"], "-dc", "-s", "-dz"]
    pipeline.main(base)
    clon = (tmp_path / "dcr_COD_1_beta.clonotypes.tsv").read_text()
    capsys.readouterr()
    pipeline.main(base + ["--cdr3-network", "--cdr3-metric", "weighted"] + flags)
    assert (tmp_path / "dcr_COD_1_beta.clonotypes.tsv").read_text() == clon
    rows = [ln.split("\t") for ln in clon.splitlines()[1:]]
    v, j, aa, dup = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [int(r[3]) for r in rows]
    R, gap, ntrim, ctrim = settings
    cost = wu.default_cost(gap, ntrim, ctrim)
    nodes = nu.Nodes(cnu.call_classes(v, j, "v"), aa, dup)
    result, stats = nu.expected_numpy(nodes, cost, R)
    assert stats["edges"] > 0 and stats["nodes_in"] == len(rows) > 300
    assert (tmp_path / "dcr_COD_1_beta.cdr3_clusters.tsv").read_text() == cnu.file_text(v, j, aa, dup, result)
    if "--write-cdr3-edges" in flags:
        assert (tmp_path / "dcr_COD_1_beta.cdr3_edges.tsv").read_text() == nu.edges_text(aa, result, cost)
    else:
        assert not (tmp_path / "dcr_COD_1_beta.cdr3_edges.tsv").exists()
    not_letters = sum(1 <= len(s) <= 32 and not wu.letters(s) for s in nodes.strings)
    assert translate.cdr3_network_stats == dict(stats, not_letters=not_letters)
    out = capsys.readouterr().out.splitlines()
    at = out.index(f"CDR3 network metric: weighted (radius {R}, gap {gap}, trim {ntrim},{ctrim}; linked CDR3s may differ in length)")
    assert f"{stats['edges']:,} pairs within radius {R}" in out[at + 1]
    assert out[at + 2] == f"CDR3 network: {not_letters:,} clonotypes took no part for a byte outside A..Z"
