"""`match` through the HIP path: dcrx_cdr3_index_create and dcrx_cdr3_match_run against the contract written in Python
(tests/cdr3_match_util.py) — degree, the CSR of hits, the targets' totals and the statistics, exactly — on degenerate inputs,
every edit position, tile and block edges on either side, classes and reach, one index under many runs, one larger table; the
primitive's work space and hit rules; and the sub-command end to end."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import pipeline
from tests import cdr3_lev_util as lu
from tests import cdr3_match_util as mu
from tests import cdr3_network_util as cnu

pytestmark = pytest.mark.gpu

ALL = [(D, metric) for metric in mu.METRICS for D in (0, 1, 2)]


def _check(case, D, metric, reference=None):
    want = (reference or mu.expected_match_naive)(case, D, metric)
    mu.assert_same(mu.native_match(case, D, metric), want, (D, metric))
    return want


# ---- degenerate inputs ----

@pytest.mark.parametrize("D,metric", ALL)
def test_no_query_no_target_one_of_each(D, metric):
    assert _check(mu.Case([], [], [], []), D, metric)["stats"]["hits"] == 0
    assert _check(mu.Case([0, 1], ["CASSF", "CASSY"], [], []), D, metric)["stats"]["targets"] == 2
    assert _check(mu.Case([], [], [0, 1], ["CASSF", "CASSY"]), D, metric)["stats"]["queries"] == 2
    assert _check(mu.Case([7], ["CASSF"], [7], ["CASSF"]), D, metric)["stats"]["hits"] == 1      # the same bytes are a hit
    assert _check(mu.Case([7], ["CASSF"], [7], ["CASSY"]), D, metric)["stats"]["hits"] == (D >= 1)
    assert _check(mu.Case([7], ["CASSF"], [8], ["CASSF"]), D, metric)["stats"]["hits"] == 0      # two classes
    assert _check(mu.Case([7], ["CASSF"], [7], ["CASSLF"]), D, metric)["stats"]["hits"] == (D >= 1 and metric == "levenshtein")


@pytest.mark.parametrize("name", ["no_target_in_reach", "no_query_in_reach"])
def test_every_node_of_one_side_out_of_reach(name):
    case = mu.constructed()[name]
    for D, metric in ((0, "hamming"), (2, "levenshtein")):
        st = _check(case, D, metric)["stats"]
        assert st["hits"] == 0 and st["queries_out_of_reach"] + st["targets_out_of_reach"] == 4


# ---- every edit position ----

@pytest.mark.parametrize("L", mu.EDIT_LENGTHS)
def test_every_edit_position(L):
    case = mu.every_edit(L)      # (its premise: every single edit in reach is a Levenshtein hit, the substitutions Hamming hits)
    for D, metric in ALL:
        _check(case, D, metric)
        _check(case.swapped(), D, metric)


def test_bytes_are_compared_as_they_are():
    case = mu.raw_bytes()
    for D, metric in ALL:
        _check(case, D, metric)
        _check(case.swapped(), D, metric)


# ---- tile and block edges, buckets one side lacks, many buckets in one block, a class across a tile ----

CONSTRUCTED = None


def _constructed(name):
    global CONSTRUCTED
    if CONSTRUCTED is None:
        CONSTRUCTED = mu.constructed()
    return CONSTRUCTED[name]


@pytest.mark.parametrize("name", [f"{side}_{n}" for side in ("targets", "queries") for n in (255, 256, 257, 513)] + ["queries_1500"])
def test_one_bucket_across_tile_and_block_edges(name):
    case = _constructed(name)
    for D, metric in ((0, "hamming"), (1, "hamming"), (2, "hamming"), (1, "levenshtein"), (2, "levenshtein")):
        want = _check(case, D, metric)
        assert want["stats"]["hits"] > 0


@pytest.mark.parametrize("name", ["gaps_t_first", "gaps_t_last", "gaps_q_first", "gaps_q_last", "many_buckets", "buckets_across_blocks",
                                  "lev_straddle"])
def test_buckets_one_side_lacks_and_many_buckets(name):
    case = _constructed(name)
    ref = mu.Reference(case)
    for D, metric in ((1, "hamming"), (2, "hamming"), (1, "levenshtein"), (2, "levenshtein")):
        _check(case, D, metric, lambda c, d, m: ref.expected(d, m))
    swapped = case.swapped()
    ref = mu.Reference(swapped)
    for D, metric in ((1, "hamming"), (2, "levenshtein")):
        _check(swapped, D, metric, lambda c, d, m: ref.expected(d, m))


@pytest.mark.parametrize("k", range(len(cnu.CLASS_BIT_PAIRS)))
def test_classes_that_differ_in_one_bit_and_nodes_out_of_reach(k):
    case = _constructed(f"class_bits_{k}")
    for D, metric in ALL:
        want = _check(case, D, metric)
        hits = [(i, int(j)) for i in range(len(case.q_strings)) for j in want["hit"][int(want["hit_off"][i]):int(want["hit_off"][i + 1])]]
        assert hits and all(case.q_classes[i] == case.t_classes[j] for i, j in hits)


# ---- the walk's two sides: a table against an index of itself, and the network of that table ----

SELF_SIZES = (1, 255, 256, 257, 513)
_self_memo = {}


def _self_table(n, spread, metric):
    """(classes, strings, sorted position of every node in the walk's bucket order): n strings of the family generators at
    length 13 (substitutions alone under hamming, indels too under levenshtein) in one class or spread over three; at 513 a few
    nodes out of reach are mixed in.  Above 256 nodes the three nodes that sort to positions 254, 255 and 256 are given one
    family of three (a string and two strings one substitution from it), so that the tile's edge runs through a row whatever
    the generator drew."""
    strings = (cnu.families if metric == "hamming" else lu.families_indel)(n, seed=100 + n, length=13)
    if n == 513:
        for k, s in ((3, ""), (200, "A" * 33), (256, ""), (400, "C" * 40), (512, "A" * 33)):
            strings[k] = s
    classes = [(5 * k + k // 7) % 3 for k in range(n)] if spread else [4] * n

    def positions():
        bs = cnu.as_bytes(strings)
        bucket = [(not mu.in_reach(s), c, len(s) if metric == "hamming" else 0) for c, s in zip(classes, bs)]
        order = sorted(range(n), key=lambda k: bucket[k])      # (stable: a bucket stays in rank order, nodes out of reach last)
        pos = [0] * n
        for p, k in enumerate(order):
            pos[k] = p
        return order, pos
    if n > 256:
        before, _ = positions()
        for k, s in zip(before[254:257], ("CASSLGQAYEQYF", "CASALGQAYEQYF", "CASSLGQAYEQFF")):
            strings[k] = s
    return classes, strings, positions()[1]


def _self_network(n, spread, D, metric):
    """The contract's network of the table, made once per (n, spread, D, metric), with the premise checked on it."""
    key = (n, spread, D, metric)
    if key not in _self_memo:
        classes, strings, pos = _self_table(n, spread, metric)
        expected = cnu.expected_network if metric == "hamming" else lu.expected_lev_network
        net, stats = expected(classes, strings, [1] * n, D)
        rows = [net["adj"][int(net["adj_off"][i]):int(net["adj_off"][i + 1])].tolist() for i in range(n)]
        if n >= 255:
            assert stats["edges"] > 20, key
        if n > 256:      # (up to 256 nodes there is no sorted position at or above 256: the table is one tile)
            assert any(min(pos[j] for j in r) < 256 <= max(pos[j] for j in r) for r in rows if r), key
        _self_memo[key] = (classes, strings, net, rows)
    return _self_memo[key]


@pytest.mark.parametrize("spread", (False, True), ids=("one_class", "three_classes"))
@pytest.mark.parametrize("n", SELF_SIZES)
def test_a_table_against_itself_is_its_network_with_every_node_in_its_own_row(n, spread):
    """The bipartite side of the walk against the one-table side: matching X against an index of X gives, row by row, the
    network's adjacency row with the node's own rank inserted in ascending order — for every node in reach; a node out of reach
    has neither —, and so the degrees and the offsets.  The premise (more than 20 edges from 255 nodes on; above 256 nodes a row
    with neighbours on both sides of sorted position 256, the tile's edge) is checked on the Python contract before any device
    call, under every (D, metric)."""
    runs = [(D, metric) for metric in mu.METRICS for D in (1, 2)]
    for D, metric in runs:
        _self_network(n, spread, D, metric)
    for D, metric in runs:
        classes, strings, want_net, rows = _self_network(n, spread, D, metric)
        off, text = cnu.node_text(strings)
        bs = cnu.as_bytes(strings)
        net, _ = nat.cdr3_network(classes, off, text, [1] * n, D, want_edges=True, metric=metric)
        got = mu.native_match(mu.Case(classes, strings, classes, strings), D, metric)
        want_rows = [sorted(r + [i]) if mu.in_reach(bs[i]) else [] for i, r in enumerate(rows)]
        assert all(not r for r, s in zip(rows, bs) if not mu.in_reach(s))
        adj_off, hit_off = np.asarray(net["adj_off"], np.uint64), np.asarray(got["hit_off"], np.uint64)
        reach_before = np.concatenate([[0], np.cumsum([mu.in_reach(s) for s in bs])]).astype(np.uint64)
        what = (n, spread, D, metric)
        assert np.array_equal(adj_off, want_net["adj_off"]) and np.array_equal(hit_off, adj_off + reach_before), what
        assert np.array_equal(np.asarray(got["degree"], np.uint64), np.asarray(net["degree"], np.uint64) + np.diff(reach_before)), what
        for i in range(n):
            a = np.asarray(net["adj"][int(adj_off[i]):int(adj_off[i + 1])]).tolist()
            h = np.asarray(got["hit"][int(hit_off[i]):int(hit_off[i + 1])]).tolist()
            assert a == rows[i] and h == want_rows[i] and (h == sorted(a + [i]) if mu.in_reach(bs[i]) else not a and not h), (what, i)


# ---- the primitive ----

def _primitive(index, case, D, metric, work_bytes=None, hit_cap=None, pattern=0xA5, twice=False):
    """dcrx_cdr3_match_device over buffers and a stream of the caller's: (degree, hit_off, the whole hit buffer, need, cap)."""
    _, (qc, off, text, _) = mu.native_args(case)
    m = len(qc)
    d_cls, d_off = nat.DeviceBuffer.from_host(qc), nat.DeviceBuffer.from_host(off)
    d_text = nat.DeviceBuffer.from_host(np.frombuffer(text + b"\0", np.uint8))
    d_deg, d_hit_off, d_need = nat.DeviceBuffer(max(16, m * 4)), nat.DeviceBuffer((m + 1) * 8), nat.DeviceBuffer(16)
    wb = nat.cdr3_match_work_bytes(m, len(text), metric) if work_bytes is None else work_bytes
    assert wb > m * 32 or work_bytes is not None
    d_work = nat.DeviceBuffer(max(256, wb))
    stream = C.c_void_p()
    nat.check(nat.lib().dcrx_stream_create(C.byref(stream)))
    try:
        # sized first (hit_cap 0, no hits), then written into `hit_cap` entries (default: exactly the need): two calls in a row
        nat.cdr3_match_device(index, m, d_cls, d_off, d_text, len(text), D, d_deg, d_hit_off, None, 0, d_need, d_work, wb, stream, metric)
        nat.check(nat.lib().dcrx_stream_synchronize(stream))
        need = int(d_need.to_host(np.uint64, 1)[0])
        cap = need if hit_cap is None else hit_cap(need)
        room = max(need, cap) + 64
        d_hit = nat.DeviceBuffer.from_host(np.full(room * 4, pattern, np.uint8))
        for _ in range(2 if twice else 1):
            nat.cdr3_match_device(index, m, d_cls, d_off, d_text, len(text), D, d_deg, d_hit_off, d_hit, cap, d_need, d_work, wb, stream,
                                  metric)
        nat.check(nat.lib().dcrx_stream_synchronize(stream))
    finally:
        nat.lib().dcrx_stream_destroy(stream)
    assert int(d_need.to_host(np.uint64, 1)[0]) == need
    return d_deg.to_host(np.uint32, m), d_hit_off.to_host(np.uint64, m + 1), d_hit.to_host(np.uint32, room), need, cap


@pytest.mark.parametrize("metric", mu.METRICS)
def test_primitive_work_space_and_hit_rules(metric):
    case = mu.classed(*mu.random_case(700, 1500, 3, 1, seed=9, length=(12, 14)), "v")
    want = mu.Reference(case).expected(2, metric)
    t_args, (_, _, text, _) = mu.native_args(case)
    assert nat.cdr3_match_work_bytes(1 << 30, 0, metric) == 0 and nat.cdr3_match_work_bytes(10, 0, 7) == 0
    assert nat.cdr3_match_work_bytes(1500, 0, "levenshtein") > nat.cdr3_match_work_bytes(1500, 0, "hamming") > 0
    index = nat.Cdr3Index(*t_args)
    try:
        assert index.info() == {"targets": 700, "out_of_reach": 0, "device_bytes": index.info()["device_bytes"]}
        assert index.info()["device_bytes"] >= 92 * 700
        with pytest.raises(nat.DcrxError, match="work space is smaller") as e:
            _primitive(index, case, 2, metric, work_bytes=nat.cdr3_match_work_bytes(1500, len(text), metric) - 1)
        assert e.value.code == -1
        filler = 0xA5A5A5A5
        # hit_cap 0 with no buffer gave the need; the exact cap: the CSR of the contract; two calls in a row on the caller's stream
        deg, hit_off, hit, need, cap = _primitive(index, case, 2, metric, twice=True)
        assert need == cap == want["stats"]["hits"] == int(hit_off[-1]) and need > 200
        assert np.array_equal(deg, want["degree"]) and np.array_equal(hit_off, want["hit_off"]) and np.array_equal(hit[:need], want["hit"])
        assert (hit[need:] == filler).all()
        # one short, and half the need: the same need, nothing behind the cap is touched, and every slot in front of it — each
        # belongs to some query's row — is written and right
        for short in (lambda n: n - 1, lambda n: n // 2):
            deg2, hit_off2, hit2, need2, cap2 = _primitive(index, case, 2, metric, hit_cap=short)
            assert need2 == need and cap2 == short(need) and np.array_equal(deg2, deg) and np.array_equal(hit_off2, hit_off)
            assert (hit2[cap2:] == filler).all()
            assert (hit2[:cap2] != filler).all() and np.array_equal(hit2[:cap2], want["hit"][:cap2])
    finally:
        index.close()


def test_refusals_of_the_entries():
    index = nat.Cdr3Index([0], *cnu.node_text(["CASSF"]))
    try:
        off, text = cnu.node_text(["CASSF"])
        with pytest.raises(nat.DcrxError, match="distance is 0, 1 or 2") as e:
            nat.cdr3_match(index, [0], off, text, [1], 3)
        assert e.value.code == -1
        with pytest.raises(nat.DcrxError, match="metric"):
            nat.cdr3_match(index, [0], off, text, [1], 1, metric=2)
        with pytest.raises(nat.DcrxError, match="backwards"):
            nat.cdr3_match(index, [0, 0], np.array([0, 5, 3], np.uint64), text, [1, 1], 1)
    finally:
        index.close()
    with pytest.raises(nat.DcrxError, match="backwards"):
        nat.Cdr3Index([0, 0], np.array([0, 5, 3], np.uint64), b"CASSF")


# ---- one index, many runs ----

def test_one_index_serves_two_tables_both_metrics_and_every_distance_in_any_order():
    ta = mu.random_case(500, 800, 3, 2, seed=31)
    tb = mu.random_case(500, 700, 3, 2, seed=32)
    a = mu.classed(*ta, "vj")
    classes = cnu.call_classes(ta[1] + tb[4], ta[2] + tb[5], "vj")      # the second table's queries against the FIRST's targets
    b = mu.Case(a.t_classes, a.t_strings, classes[500:], tb[3])
    refs = {"a": mu.Reference(a), "b": mu.Reference(b)}
    t_args, qa = mu.native_args(a)
    _, qb = mu.native_args(b)
    index = nat.Cdr3Index(*t_args)
    try:
        runs = [(n, D, metric) for n in ("a", "b") for D, metric in ALL]
        for order in (runs, runs[::-1], runs[1::2] + runs[::2]):
            for n, D, metric in order:
                got = nat.cdr3_match(index, *(qa if n == "a" else qb), D, metric)
                mu.assert_same(got, refs[n].expected(D, metric), (n, D, metric))
    finally:
        index.close()
    assert refs["a"].expected(2, "levenshtein")["stats"]["hits"] > refs["a"].expected(2, "hamming")["stats"]["hits"] > 0


def test_three_hundred_queries_on_one_target_and_the_weight_sum():
    big = (1 << 64) - 1
    weights = [big - 299 * 7] + [7] * 299                         # the sum is 2^64 - 1: accepted, and one target carries it
    case = mu.Case([0, 0], ["CASSLGQAYEQYF", "CAWWWWWWWWWWF"], [0] * 300, ["CASSLGQAYEQYF"] * 300, weights)
    want = _check(case, 1, "hamming")
    assert want["t_queries"].tolist() == [300, 0] and [int(x) for x in want["t_weight"]] == [big, 0]
    assert want["stats"]["queries_hit_weight"] == big and want["stats"]["targets_hit"] == 1
    case.weights[1] += 1                                          # exactly 2^64: refused, on the host
    with pytest.raises(nat.DcrxError, match="2\\^64") as e:
        mu.native_match(case, 1, "hamming")
    assert e.value.code == nat.E_UNSUPPORTED
    # no target: the refusal does not depend on the device being needed
    with pytest.raises(nat.DcrxError, match="2\\^64"):
        mu.native_match(mu.Case([], [], case.q_classes, case.q_strings, case.weights), 1, "hamming")


# ---- one larger table ----

@pytest.fixture(scope="module")
def big():
    """200 000 queries against 20 000 targets in 60 classes (12 V x 5 J), drawn from 12 000 distinct strings of 11 to 16 letters
    in families with substitutions, insertions and deletions; the reference and the index are made once, and the index is closed
    behind the module's last test."""
    case = mu.classed(*mu.random_case(20000, 200000, 12, 5, seed=77, pool=12000), "vj")
    assert len(set(case.t_classes) | set(case.q_classes)) == 60
    t_args, q_args = mu.native_args(case)
    index = nat.Cdr3Index(*t_args)
    try:
        yield {"ref": mu.Reference(case), "index": index, "q_args": q_args}
    finally:
        index.close()


@pytest.mark.parametrize("D,metric", [(1, "hamming"), (2, "hamming"), (1, "levenshtein"), (2, "levenshtein")])
def test_larger_table_equals_the_reference(big, D, metric):
    want = big["ref"].expected(D, metric)
    st = want["stats"]
    # the reference itself shows hits at every distance 0 .. D, and queries and targets without any
    assert big["ref"].distances_seen(D, metric) == set(range(D + 1))
    assert 1000 < st["queries_hit"] < st["queries"] and 100 < st["targets_hit"] < st["targets"]
    mu.assert_same(nat.cdr3_match(big["index"], *big["q_args"], D, metric), want, (D, metric))


# ---- the sub-command, end to end ----

def _clonotypes_text(rows) -> bytes:
    lines = ["\t".join(nat.CLONOTYPE_COLUMNS)]
    for v, j, aa, dup in rows:
        lines.append("\t".join([v, j, aa, str(dup)] + ["0"] * (len(nat.CLONOTYPE_COLUMNS) - 4)))
    return ("\n".join(lines) + "\n").encode("latin-1")


def _tables(seed):
    ts, tv, tj, qs, qv, qj = mu.random_case(400, 900, 4, 2, seed=seed)
    qs[5], ts[7] = "A" * 33, ""                                    # out of reach on either side
    half = len(qs) // 2
    samples = [("S1", list(zip(qv[:half], qj[:half], qs[:half], range(1, half + 1)))),
               ("S2", list(zip(qv[half:], qj[half:], qs[half:], range(3, 3 + len(qs) - half))))]
    return ts, tv, tj, samples


@pytest.mark.parametrize("D,metric,mode", [(1, "hamming", "v"), (2, "levenshtein", "vj"), (0, "hamming", "none")])
def test_sub_command_with_renamed_columns_byte_for_byte(D, metric, mode, tmp_path, capsys):
    ts, tv, tj, samples = _tables(seed=41)
    db_header = [b"Epitope", b"CDR3", b"V", b"J"]
    db_lines = [b"\t".join([b"EPI%d" % (k % 9), t.encode("latin-1"), v.encode(), j.encode()]) for k, (t, v, j) in enumerate(zip(ts, tv, tj))]
    db = tmp_path / "known.tsv.gz"
    with gzip.open(db, "wb") as fh:
        fh.write(b"\t".join(db_header) + b"\n" + b"\n".join(db_lines) + b"\n")
    files = []
    for name, rows in samples:
        files.append(str(tmp_path / (name + ".clonotypes.tsv")))
        open(files[-1], "wb").write(_clonotypes_text(rows))
    out = str(tmp_path / "out") + os.sep
    os.makedirs(out)
    pipeline.main(["match", "-in", *files, "-db", str(db), "-op", out, "-pf", "m_", "-dz", "--cdr3-distance", str(D), "--cdr3-metric", metric,
                   "--cdr3-class", mode, "--db-cdr3-column", "CDR3", "--db-v-column", "V", "--db-j-column", "J"])
    assert sorted(os.listdir(out)) == ["m_S1.cdr3_matches.tsv", "m_S2.cdr3_matches.tsv", "m_match_targets.tsv"]
    results = []
    all_v, all_j = tv + [r[0] for _, rows in samples for r in rows], tj + [r[1] for _, rows in samples for r in rows]
    classes = cnu.call_classes(all_v, all_j, mode)
    at = len(ts)
    for name, rows in samples:
        case = mu.Case(classes[:len(ts)], ts, classes[at:at + len(rows)], [r[2] for r in rows], [r[3] for r in rows])
        at += len(rows)
        want = mu.expected_match_naive(case, D, metric)
        assert want["stats"]["hits"] > 0
        results.append(want)
        text = mu.matches_text([r[0] for r in rows], [r[1] for r in rows], case, want, db_header, db_lines, metric)
        assert open(out + f"m_{name}.cdr3_matches.tsv", "rb").read() == text, name
    assert open(out + "m_match_targets.tsv", "rb").read() == mu.targets_text(["S1", "S2"], db_header, db_lines, results)
    printed = capsys.readouterr().out.splitlines()
    assert len(printed) == 2 and printed[0].startswith("Match of S1 against 400 database entries")


@pytest.mark.parametrize("D,metric", [(1, "hamming"), (2, "hamming"), (1, "levenshtein"), (2, "levenshtein")])
def test_a_sample_as_database_equals_the_cross_edges_of_the_network(D, metric, tmp_path):
    """`match -in A -db B.clonotypes.tsv` against the route there was before: nat.cdr3_network over A and B concatenated, the
    edges between an A node and a B node kept."""
    ts, tv, tj, samples = _tables(seed=43)
    a_rows = samples[0][1]
    b_rows = list(zip(tv, tj, ts, range(1, len(ts) + 1)))
    a, b = str(tmp_path / "A.clonotypes.tsv"), str(tmp_path / "B.clonotypes.tsv")
    open(a, "wb").write(_clonotypes_text(a_rows))
    open(b, "wb").write(_clonotypes_text(b_rows))
    out = str(tmp_path / "out") + os.sep
    os.makedirs(out)
    pipeline.main(["match", "-in", a, "-db", b, "-op", out, "-pf", "", "-dz", "--cdr3-distance", str(D), "--cdr3-metric", metric])
    lines = open(out + "A.cdr3_matches.tsv", "rb").read().splitlines()[1:]
    got = {(int(f[0]), int(f[5])) for f in (ln.split(b"\t") for ln in lines)}
    n_a = len(a_rows)
    classes = cnu.call_classes([r[0] for r in a_rows] + tv, [r[1] for r in a_rows] + tj, "v")
    off, text = cnu.node_text([r[2] for r in a_rows] + ts)
    net, _ = nat.cdr3_network(classes, off, text, [1] * len(classes), D, want_edges=True, metric=metric)
    cross = {(i, int(j) - n_a) for i in range(n_a) for j in net["adj"][int(net["adj_off"][i]):int(net["adj_off"][i + 1])] if j >= n_a}
    assert got == cross and len(got) > 50
